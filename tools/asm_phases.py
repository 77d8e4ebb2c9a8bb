"""Static instruction mix of k_ct_mul_fresh per phase: compiles csrc/k_mul_fresh.hip with
-DPVAC_ASM_MARKS (the PHASE_STAMP sites become asm comments) and counts VALU / SALU / LDS /
VMEM instructions between consecutive marks. Diagnostic only (CPU, no GPU).
With --blocks, also one line per basic block (label, the phase mark it follows, its counts and the
branch that ends it): following a shape's path through the blocks gives a per-wave static count.
Usage: python tools/asm_phases.py [--blocks] [extra hipcc flags]"""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.environ.get("SRC") or os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "csrc", "k_mul_fresh.hip")   # SRC: another revision
OUT = "/tmp/k_mul_fresh_marks.s"


def main():
    flags = [a for a in sys.argv[1:] if a != "--blocks"]
    blocks = [] if "--blocks" in sys.argv[1:] else None   # [label, mark, Counter, last branch]
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "--offload-arch=gfx950", "-x", "hip", "--cuda-device-only",
           "-S", "-DPVAC_ASM_MARKS", *flags, SRC, "-o", OUT]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    lines = open(OUT).read().splitlines()
    kern = os.environ.get("KERNEL", "k_ct_mul_fresh3")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + kern + r"I\S*:", l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    cur = "entry"
    cnt = collections.OrderedDict()
    for l in lines[start:end]:
        m = re.search(r"PVAC_MARK (\d+)", l)
        if m:
            cur = m.group(1)
            if blocks is not None:   # a mark splits its block, so every row lies in one phase
                blocks.append([f"(mark {cur})", cur, collections.Counter(), ""])
            continue
        t = l.strip().split()
        if blocks is not None and t and t[0].endswith(":") and not t[0].startswith(";"):
            note = l.split(";", 1)[1].strip() if ";" in l else ""
            name = t[0][:-1] if t[0].startswith(".") else "(kernel entry)"
            blocks.append([name + (" " + note if "Loop" in note else ""), cur, collections.Counter(), ""])
        if not t or t[0].startswith((";", ".")) or t[0].endswith(":"):
            continue
        op = t[0]
        cls = ("valu" if op.startswith("v_") else "salu" if op.startswith("s_") and not op.startswith(("s_waitcnt", "s_barrier", "s_cbranch", "s_branch", "s_load", "s_buffer")) else
               "lds" if op.startswith("ds_") else "vmem" if op.startswith(("global_", "buffer_", "flat_")) else
               "smem" if op.startswith(("s_load", "s_buffer")) else "ctl")
        d = cnt.setdefault(cur, collections.Counter())
        d[cls] += 1
        if blocks is not None:
            if not blocks:
                blocks.append(["(entry)", cur, collections.Counter(), ""])
            blocks[-1][2][cls] += 1
            if op.startswith(("s_cbranch", "s_branch")):
                blocks[-1][3] = " ".join(t[:2])
    tot = collections.Counter()
    for k, d in cnt.items():
        tot.update(d)
        print(f"after mark {k:>5}: " + " ".join(f"{c}={d[c]}" for c in ("valu", "salu", "lds", "vmem", "smem", "ctl")))
    if blocks is not None:
        print("basic blocks (label, after mark, counts, last branch):")
        for label, mark, d, br in blocks:
            if sum(d.values()):
                print(f"  {label:<44} {mark:>5}  " + " ".join(f"{c}={d[c]:<4}" for c in ("valu", "salu", "lds", "vmem", "smem", "ctl"))
                      + "  " + br)
    print("total:          " + " ".join(f"{c}={tot[c]}" for c in ("valu", "salu", "lds", "vmem", "smem", "ctl")))


if __name__ == "__main__":
    main()
