"""Timing of the device .ct codec (GPU box): pvac_hip_ct_image_write / _parse on three shapes,
  (a) 2^16 fresh ciphers with sigma (about 2.8 GB of image),
  (b) 2^20 fresh ciphers, weights only,
  (c) one chunk of depth-8 chain results (64 inputs, capacity-padded, weights only).
Per shape: device time of ct_image_write and ct_image_parse from the engine's HIP-event timers (median
after warm-up), image bytes per second, and the share of the device-to-device copy rate of the same
byte count measured in the same process (the kernels move each byte once in and once out, so a copy is
their ceiling); then, once, the end-to-end wall time of codec.save_ct_device / load_ct_device against
codec.save_ct / load_ct on the same batch, files and arrays compared. Prints one JSON line; --out also
writes it to a file.
Usage: python tools/exp_codec.py [--reps 5] [--scale 1.0] [--no-host] [--out profiles/codec/exp_codec.json]"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pvac_hfhe_cppbyv_amd import DeviceBatch, Engine, codec  # noqa: E402


def lib_sha256():
    with open(os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip.so"), "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def timed(eng, label, call, reps, warm=1):
    """Median and minimum device milliseconds of `call` under the library's timing label."""
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


def copy_ms(nbytes, device, reps, warm=1):
    """Median milliseconds of a device-to-device copy of nbytes (read once, written once)."""
    src = torch.empty(nbytes, dtype=torch.uint8, device=device)
    dst = torch.empty_like(src)
    ms = []
    for k in range(warm + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        if k >= warm:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kept_layers(L):
    """Layer rows as the format keeps them: PROD without its seed, BASE without pa / pb, pad 0."""
    L = L.clone()
    prod = (L[:, 0] & 0xFFFFFFFF) == 1
    L[prod, 2:] = 0
    L[:, 1] &= 0xFFFFFFFF
    L[~prod, 0] &= 0xFFFFFFFF
    L[~prod, 1] = 0
    return L


def same_batch(a, b):
    n = a.n
    ok = all(torch.equal(getattr(a, f)[:n], getattr(b, f)[:n]) for f in ("l_off", "l_cnt", "e_off", "e_cnt"))
    nl, ne = int(a.l_cnt[:n].sum().item()), int(a.e_cnt[:n].sum().item())
    ok = ok and torch.equal(kept_layers(a.layers[:nl]), kept_layers(b.layers[:nl]))
    for f in ("meta", "w_lo", "w_hi"):
        ok = ok and torch.equal(getattr(a, f)[:ne], getattr(b, f)[:ne])
    if a.sigma is not None or b.sigma is not None:
        ok = ok and a.sigma is not None and b.sigma is not None and torch.equal(a.sigma[:ne], b.sigma[:ne])
    return bool(ok)


def shape(eng, name, X, reps, host, tmp):
    sigma = X.sigma is not None
    bits = 8192
    image, pos = eng.ct_image(X, bits, return_pos=True)
    nbytes = image.numel()
    n = X.n
    nl, ne = int(X.l_cnt[:n].sum().item()), int(X.e_cnt[:n].sum().item())
    res = {"shape": name, "ciphers": n, "layers": nl, "edges": ne, "sigma": sigma, "image_bytes": nbytes}
    before = eng.ct_image_path_counts()
    w_ms, w_min = timed(eng, "ct_image_write", lambda: eng.ct_image(X, bits), reps)
    out = DeviceBatch.empty(n, nl, ne, eng.device)
    if sigma:
        out.sigma = torch.empty((max(ne, 1), 128), dtype=torch.int64, device=eng.device)
    pbits = bits if sigma else 0
    p_ms, p_min = timed(eng, "ct_image_parse", lambda: eng.ct_from_image(image, pos, n, pbits, nl, ne, out=out), reps)
    after = eng.ct_image_path_counts()
    c_ms = copy_ms(nbytes, eng.device, reps)
    res["ms"] = {"write": round(w_ms, 4), "write_min": round(w_min, 4), "parse": round(p_ms, 4), "parse_min": round(p_min, 4),
                 "copy": round(c_ms, 4)}
    res["GB_per_s"] = {"write": round(nbytes / w_ms / 1e6, 1), "parse": round(nbytes / p_ms / 1e6, 1),
                       "copy": round(nbytes / c_ms / 1e6, 1)}
    res["of_copy_rate"] = {"write": round(c_ms / w_ms, 3), "parse": round(c_ms / p_ms, 3)}
    res["paths"] = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    res["round_trip_equals_pack"] = same_batch(out, eng.pack(X))
    del out, image
    if host:
        fd, fh = os.path.join(tmp, name + "_dev.ct"), os.path.join(tmp, name + "_host.ct")
        sd_ms, _ = wall(lambda: codec.save_ct_device(eng, X, fd, bits))
        sh_ms, _ = wall(lambda: codec.save_ct(X, fh, bits))
        sha = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()
        res["files_equal"] = sha(fd) == sha(fh)
        os.remove(fh)
        ld_ms, D = wall(lambda: codec.load_ct_device(eng, fd, sigma=sigma))
        lh_ms, H = wall(lambda: codec.load_ct(fd, eng.device, sigma=sigma))
        res["loads_equal"] = same_batch(D, H)
        os.remove(fd)
        res["wall_ms"] = {"save_ct_device": round(sd_ms, 1), "save_ct": round(sh_ms, 1), "load_ct_device": round(ld_ms, 1),
                          "load_ct": round(lh_ms, 1)}
        res["speedup"] = {"save": round(sh_ms / sd_ms, 2), "load": round(lh_ms / ld_ms, 2)}
    print(json.dumps(res), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the two fresh shapes (a quick run)")
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--no-host", action="store_true", help="skip the end-to-end comparison with the host codec")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("exp_codec: needs a GPU")
    eng = Engine(device=0, canon_tag=0x5EED0005)
    eng.timing(True)
    res = {"library_sha256": lib_sha256(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "shapes": []}
    k = lambda x: max(int(x * a.scale), 64)
    with tempfile.TemporaryDirectory() as tmp:
        X = eng.gen_fresh(k(1 << 16), 21, 20)
        X.sigma = torch.empty((X.meta.shape[0], 128), dtype=torch.int64, device=eng.device)
        eng.fill_random(X.sigma, 22)
        res["shapes"].append(shape(eng, "fresh_sigma", X, a.reps, not a.no_host, tmp))
        del X
        res["shapes"].append(shape(eng, "fresh_weights", eng.gen_fresh(k(1 << 20), 23, 20), a.reps, not a.no_host, tmp))
        x = eng.gen_fresh(a.chains, 12, 20)
        c = x
        for d in range(8):
            c = eng.ct_mul(c, x, nonce_seed=0x5EED0100 + d)
        res["shapes"].append(shape(eng, f"depth8_chain_chunk_{a.chains}", c, a.reps, not a.no_host, tmp))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
