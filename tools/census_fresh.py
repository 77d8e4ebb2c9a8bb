"""Workgroup residency of the fresh ct_mul kernel from the CENSUS build (lib/libpvac_hip_census.so):
per-workgroup start / end times, CU ids and the SIMD that holds each of its waves. Diagnostic only: never used by tests or bench.py.
Usage (GPU box): python tools/census_fresh.py [pairs [library]]"""
import ctypes as C
import collections
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from pvac_hfhe_cppbyv_amd import Engine, load_library  # noqa: E402


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    lib = load_library(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "lib", "libpvac_hip_census.so"))
    lib.pvac_hip_diag_census.argtypes = [C.c_void_p, C.c_size_t]
    eng = Engine(device=0, canon_tag=0x5EED0003, lib=lib)
    A = eng.gen_fresh(n, 0x5EED0003, 20)
    B = eng.gen_fresh(n, 0x5EED0004, 20)
    for _ in range(2):
        Cb, plan = eng.ct_mul_plan(A, B)
        nonces = eng.fill_nonces(A, B, Cb, plan, 1)
        eng.ct_mul(A, B, nonces=nonces, C_=Cb, plan=plan)
    torch.cuda.synchronize()
    row = 3 + 8   # start, end, pairs, then HW_ID | XCC_ID << 32 of waves 0..7
    st = np.zeros(4096 * row, np.uint64)
    assert lib.pvac_hip_diag_census(st.ctypes.data_as(C.c_void_p), st.size) == 0
    st = st.reshape(4096, row)
    used = st[st[:, 1] > 0]
    t0 = used[:, 0].min()
    start = (used[:, 0] - t0) / 100.0   # us (100 MHz)
    end = (used[:, 1] - t0) / 100.0
    print("workgroups", len(used), "kernel span us %.1f" % end.max())
    print("start us: min %.1f p50 %.1f p90 %.1f max %.1f" % tuple(np.percentile(start, [0, 50, 90, 100])))
    print("end   us: min %.1f p50 %.1f p90 %.1f max %.1f" % tuple(np.percentile(end, [0, 50, 90, 100])))
    print("pairs per wg: min %d max %d" % (used[:, 2].min(), used[:, 2].max()))
    hw = used[:, 3].astype(np.int64)   # wave 0's
    cu = (hw >> 8) & 0xF
    sh = (hw >> 12) & 1
    se = (hw >> 13) & 0x7
    xcc = (hw >> 32) & 0xF
    key = list(zip(xcc, se, sh, cu))
    cnt = collections.Counter(key)
    late = start > 0.25 * end.max()
    print("distinct (xcc, se, sh, cu) ids", len(cnt), "max wg per id", max(cnt.values()), "late starters", int(late.sum()))
    # wave -> SIMD placement: HW_ID bits 5:4 of every wave's lane 0
    simd = (used[:, 3:].astype(np.int64) >> 4) & 3   # [workgroup][wave]
    same_cu = (((used[:, 3:].astype(np.int64) >> 8) & 0xFF) == ((hw >> 8) & 0xFF)[:, None]).all()
    print("every wave of a workgroup on its wave 0's CU:", bool(same_cu))
    paired = (simd[:, :4] == simd[:, 4:]).all(axis=1)
    spread = np.array([len(set(r[:4])) == 4 for r in simd])
    print("workgroups with waves w and w + 4 on one SIMD: %d of %d; with waves 0..3 on four SIMDs: %d"
          % (int(paired.sum()), len(simd), int(spread.sum())))
    pat = collections.Counter("".join(map(str, r)) for r in simd)
    print("SIMD of waves 0..7, by pattern (count):", ", ".join(f"{k} ({v})" for k, v in pat.most_common(12)),
          "... %d patterns" % len(pat) if len(pat) > 12 else "")
    print("per CU (xcc.se.sh.cu): SIMD of waves 0..7 of each resident workgroup, in start order")
    by_cu = collections.defaultdict(list)
    for i in np.argsort(start, kind="stable"):
        by_cu[key[i]].append("".join(map(str, simd[i])))
    for k in sorted(by_cu):
        print("  %d.%d.%d.%-2d %s" % (*k, "  ".join(by_cu[k])))


if __name__ == "__main__":
    main()
