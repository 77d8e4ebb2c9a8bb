"""Static issue price of k_ct_mul_fresh3<512> per phase (CPU, no GPU).

Compiles csrc/k_mul_fresh.hip for gfx950 with -DPVAC_ASM_MARKS (the M3(n) sites become
`; PVAC_MARK n` lines), splits the kernel's ISA at the marks into P1, P2, P3, P4, P5, the staging
of the next pair, the writer and the rest, counts the VALU instructions of every segment per opcode and weights each opcode with
its measured issue cost at 8 waves per SIMD (`wps8.cycles_per_inst` of
profiles/r05/issue_probe_vcc.json). An opcode the probe did not measure is priced at the median
of the full class (every probed opcode above 3.5 cycles) and listed as unpriced.

The priced cycles of a segment are multiplied by how often a pair runs that code at the bench
shape (40 x 40 edges, 2 x 2 layers, B = 337):
  P1, P5 : the text holds U = 4 product rounds of a wave without a partial round; each of the 8
           waves runs it once and skips its empty rounds (7 of the 32 at 1,600 products), so 25
           wave-rounds -> x 25 / 4. With --rounds parent (a source from before the round classes)
           P1 is priced x 8: there every wave ran the index arithmetic and the LDS reads of all
           four rounds and skipped only the cell half of an empty one, so x 8 is an upper bound
           and x 25 / 4 a lower one for that text; P5 skipped an empty pair of rounds as now.
  loops  : P1's and P5's clamped and masked loops (products past U * 512, and every product of a
           wave with a partial round): not run at the bench shape -> x 0
  writer : one position round in the text, 21 wave-rounds (about 1,330 emit positions) -> x 21
  gate   : the writer's canonical finish and zero ballot, run only in a position round where a
           lane's top word is 0 or 0x7FFFFFFF (about 2^-30 per lane for the bench's weights) -> x 0
  stage  : stage_pair of the next pair, run by the one wave that holds its 40 edges -> x 1
  P2, P4 : the text holds KR = 2 bin rows, a pair has 8 wave-rows of bins -> x 8 / 2
  P3, rest (loop head, barriers, header decode, tail): once per wave -> x 8
The model is flat: it prices every instruction of a segment's text, whichever branch a wave
takes. P2 and P4 hold one straight-line body per bin kind (a wave runs one of them), the rest
holds the rebuild of the slot records (not run per pair) and is therefore listed without a
per-pair price, and the writer's segment ends with the clear of the cell words. The per-pair total
is a yardstick for deltas between two revisions of the source, not a time.

Usage: python tools/issue_price.py [--src FILE] [--probe FILE] [--keep-asm FILE] [extra hipcc flags]
"""
import argparse
import collections
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pvac_hfhe_cppbyv_amd", "csrc")
KERNEL = "k_ct_mul_fresh3ILi512E"
SEGMENTS = collections.OrderedDict([("1", "P1"), ("10", "P1loop"), ("2", "P2"), ("3", "P3"), ("4", "P4"), ("5", "P5"),
                                    ("11", "P5loop"), ("7", "stage"), ("6", "writer"), ("9", "gate")])
U, KR = 4, 2
# runs of a segment's text per pair (see the module text); None: not priced per pair
TRIPS = {"P1": 25 / U, "P1loop": 0.0, "P5": 25 / U, "P5loop": 0.0, "stage": 1.0, "writer": 21.0, "gate": 0.0, "P2": 8 / KR,
         "P4": 8 / KR, "P3": 8.0, "rest": None}
SUFFIX = re.compile(r"_(e32|e64|dpp|sdwa|e64_dpp)$")
# ISA opcode -> probe row, where the probe's row carries a variant in its name. The probe's plain
# v_cndmask_b32 row (22.7 cycles) timed a dependent chain through VCC, not the issue cost; the
# select is priced by the e64 row, as the issue cost table of DESIGN section 19 does.
ALIAS = {"v_addc_co_u32": "v_addc_co_u32_vcc", "v_subb_co_u32": "v_addc_co_u32_vcc", "v_sub_co_u32": "v_add_co_u32",
         "v_cndmask_b32": "v_cndmask_b32_e64", "v_subrev_u32": "v_sub_u32"}


def compile_isa(src, flags, keep):
    out = keep or os.path.join(tempfile.mkdtemp(prefix="issue_price_"), "k_mul_fresh_marks.s")
    cmd = ["/opt/rocm/bin/hipcc", "-std=c++17", "-O3", "-fPIC", "--offload-arch=gfx950", "-I", CSRC, "-x", "hip",
           "--cuda-device-only", "-S", "-DPVAC_ASM_MARKS", *flags, src, "-o", out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    return open(out).read().splitlines()


def probe_costs(path):
    ops = json.load(open(path))["ops"]
    cost = {k: v["wps8"]["cycles_per_inst"] for k, v in ops.items()}
    full = [c for k, c in cost.items() if 3.5 < c < 10.0]
    return cost, statistics.median(full)


def price_of(op, dpp, cost, full_median):
    """(cycles, priced?) of one VALU opcode as the ISA names it."""
    base = SUFFIX.sub("", op)
    if dpp and "v_mov_b32_dpp" in cost and base == "v_mov_b32":
        return cost["v_mov_b32_dpp"], True
    for name in (op, base, ALIAS.get(base, "")):
        if name in cost and not (name == "v_cndmask_b32" and cost[name] > 10.0):
            return cost[name], True
    return full_median, False


def resources(lines):
    """VGPRs, scratch bytes and spill counts of the kernel from the code object's metadata."""
    at = next(i for i, l in enumerate(lines) if ".name:" in l and KERNEL in l)
    want = {".vgpr_count": "vgprs", ".private_segment_fixed_size": "scratch_bytes", ".vgpr_spill_count": "vgpr_spills",
            ".sgpr_spill_count": "sgpr_spills", ".sgpr_count": "sgprs"}
    res = {}
    for l in lines[at + 1:]:   # a record's keys are sorted: the five wanted ones follow .name
        if l.lstrip().startswith(("- ", "amdhsa.")) or len(res) == len(want):
            break
        m = re.match(r"\s*(\.\w+):\s+(\d+)\s*$", l)
        if m and m.group(1) in want:
            res[want[m.group(1)]] = int(m.group(2))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--src", default=os.path.join(CSRC, "k_mul_fresh.hip"), help="another revision of the source")
    ap.add_argument("--probe", default=os.path.join(ROOT, "profiles", "r05", "issue_probe_vcc.json"))
    ap.add_argument("--keep-asm", default=None, help="write the marked ISA here")
    ap.add_argument("--rounds", choices=("classes", "parent"), default="classes",
                    help="parent: a source from before the round classes (P1 priced x 8, see the module text)")
    args, flags = ap.parse_known_args()
    if args.rounds == "parent":
        TRIPS["P1"] = 8.0
    cost, full_median = probe_costs(args.probe)
    lines = compile_isa(args.src, flags, args.keep_asm)
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*" + KERNEL + r"\S*:", l))
    end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
    seg = "rest"
    count = collections.OrderedDict((s, collections.Counter()) for s in [*dict.fromkeys(SEGMENTS.values()), "rest"])
    other = collections.Counter()   # non-VALU instructions per segment (reported, not priced)
    for l in lines[start:end]:
        m = re.search(r"PVAC_MARK (\d+)", l)
        if m:
            seg = SEGMENTS.get(m.group(1), "rest")
            continue
        t = l.strip().split()
        if not t or t[0].startswith((";", ".")) or t[0].endswith(":"):
            continue
        if t[0].startswith("v_"):
            dpp = any(x.startswith(("row_", "quad_perm", "wave_", "bank_mask")) for x in t[1:])
            count[seg][(t[0], dpp)] += 1
        else:
            other[seg] += 1
    unpriced = collections.Counter()
    rows = []
    per_op = collections.Counter()      # priced cycles per pair by opcode
    per_op_n = collections.Counter()    # static count by opcode
    for s, c in count.items():
        n = sum(c.values())
        cyc = 0.0
        for (op, dpp), k in c.items():
            p, ok = price_of(op, dpp, cost, full_median)
            cyc += p * k
            base = SUFFIX.sub("", op) + ("(dpp)" if dpp else "")
            per_op_n[base] += k
            if TRIPS[s] is not None:
                per_op[base] += p * k * TRIPS[s]
            if not ok:
                unpriced[SUFFIX.sub("", op)] += k
        rows.append((s, n, other[s], cyc, None if TRIPS[s] is None else cyc * TRIPS[s]))
    total = sum(r[4] for r in rows if r[4] is not None)
    print(f"source: {os.path.relpath(args.src, ROOT)}")
    print(f"probe : {os.path.relpath(args.probe, ROOT)} (wps8; full-class median {full_median:.2f} cycles)")
    print()
    print(f"{'segment':<8}{'VALU':>7}{'other':>7}{'cycles/run':>12}{'runs/pair':>11}{'cycles/pair':>13}{'share':>8}")
    for s, n, o, cyc, pp in rows:
        if n == 0 and o == 0:
            continue   # a segment this source has no mark for
        if pp is None:
            print(f"{s:<8}{n:>7}{o:>7}{cyc:>12.0f}{'-':>11}{'-':>13}{'-':>8}")
        else:
            print(f"{s:<8}{n:>7}{o:>7}{cyc:>12.0f}{TRIPS[s]:>11.2f}{pp:>13.0f}{pp / total:>8.1%}")
    print(f"{'total':<8}{sum(r[1] for r in rows):>7}{sum(r[2] for r in rows):>7}{'':>12}{'':>11}{total:>13.0f}")
    print()
    print("ten costliest opcodes (priced cycles per pair, static count in the kernel):")
    for op, cyc in per_op.most_common(10):
        print(f"  {op:<24}{cyc:>10.0f}{cyc / total:>8.1%}{per_op_n[op]:>7}")
    print()
    if unpriced:
        print("unpriced (full-class median): " + ", ".join(f"{k} x{v}" for k, v in sorted(unpriced.items())))
    else:
        print("unpriced: none")
    r = resources(lines)
    print("resources: " + ", ".join(f"{k} {r[k]}" for k in ("vgprs", "sgprs", "scratch_bytes", "vgpr_spills", "sgpr_spills") if k in r))
    return 0


if __name__ == "__main__":
    sys.exit(main())
