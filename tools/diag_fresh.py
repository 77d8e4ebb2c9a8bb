"""Per-phase wall time of k_ct_mul_fresh from the DIAGNOSTIC build (lib/libpvac_hip_diag.so,
s_memtime stamps of every wave's lane 0 per workgroup: wave 0's phases, then a wave x phase table). Diagnostic only: never used by tests or bench.py.
Usage (GPU box): python tools/diag_fresh.py [pairs [library]]"""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pvac_hfhe_cppbyv_amd import Engine, load_library  # noqa: E402

# k_ct_mul_fresh3 (default kernel): work phases end with an lgkmcnt(0) stamp, then the barrier wait
PHASES = ["loop top (header, rebuild)", "P1 key times", "  B1 wait", "P2 order", "  B2 wait", "P3 closure (wave 0)",
          "  B3 wait (scan)", "P4 positions", "  B4 wait", "P5 products", "  B5 wait", "P6 writer", "P6 reset+stage",
          "  B6 wait", "-", "-", "-", "-"]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    lib = load_library(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip_diag.so"))
    lib.pvac_hip_diag_fresh_stamps.argtypes = [C.c_void_p, C.c_size_t]
    eng = Engine(device=0, canon_tag=0x5EED0003, lib=lib)
    A = eng.gen_fresh(n, 0x5EED0003, 20)
    B = eng.gen_fresh(n, 0x5EED0004, 20)
    for _ in range(2):
        Cb, plan = eng.ct_mul_plan(A, B)
        nonces = eng.fill_nonces(A, B, Cb, plan, 1)
        eng.ct_mul(A, B, nonces=nonces, C_=Cb, plan=plan)
    torch.cuda.synchronize()
    st = np.zeros(4096 * 8 * 18, np.uint64)
    assert lib.pvac_hip_diag_fresh_stamps(st.ctypes.data_as(C.c_void_p), st.size) == 0
    st = st.reshape(4096, 8, 18)   # [workgroup][wave][phase], lane 0 of every wave
    used = st[st.sum(axis=(1, 2)) > 0]
    tot = used[:, 0, :].sum(axis=0).astype(np.float64)   # wave 0, as before the per-wave stamps
    frac = tot / tot.sum()
    per_pair = tot / n   # ticks per pair per workgroup
    print(json.dumps({"workgroups": int(used.shape[0]), "pairs": n,
                      "ticks_per_pair_per_wg": float(tot.sum() / n),
                      "phases": {PHASES[i]: {"frac": round(float(frac[i]), 4), "ticks_per_pair": round(float(per_pair[i]), 1)}
                                 for i in range(len(PHASES))}}, indent=1))
    # per wave: ticks per pair of every phase. A work phase is the wave's own time up to its
    # lgkmcnt(0) stamp, the wait that follows is the time it stood at the barrier: a wave that
    # binds a phase shows the longest work and the shortest wait
    pw = used.sum(axis=0).astype(np.float64) / n   # [wave][phase]
    live = [i for i in range(len(PHASES)) if PHASES[i] != "-"]
    print("ticks per pair, by wave (rows) and phase (columns):")
    print("wave " + " ".join(f"{PHASES[i].strip()[:9]:>9}" for i in live) + "      work      wait")
    for w in range(8):
        work = sum(pw[w, i] for i in live if "wait" not in PHASES[i])
        wait = sum(pw[w, i] for i in live if "wait" in PHASES[i])
        print(f"{w:>4} " + " ".join(f"{pw[w, i]:9.1f}" for i in live) + f" {work:9.1f} {wait:9.1f}")


if __name__ == "__main__":
    main()
