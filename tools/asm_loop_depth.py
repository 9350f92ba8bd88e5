"""Instructions of one kernel in a `hipcc -S --cuda-device-only` gfx950 listing
by loop depth and by basic block, with the AGPR moves among them (tools only).
A peeled loop shows as blocks of the enclosing depth, so the dynamic count of
one outer iteration is the sum of its depth-1 blocks plus the trip count times
the depth-2 blocks.
  python tools/asm_loop_depth.py FILE.s KERNEL_SUBSTRING [MIN_BLOCK]"""
import re
import sys
from collections import Counter

s = open(sys.argv[1]).read()
name = [n for n in re.findall(r"\n(_Z\w+):", s) if sys.argv[2] in n][0]
minblk = int(sys.argv[3]) if len(sys.argv) > 3 else 30
st = s.index("\n" + name + ":") + 1
en = s.index(".Lfunc_end", st)
depth, blocks, ops = 0, [["entry", 0, 0, 0]], {}
for ln in s[st:en].splitlines():
    if re.match(r"^\.LBB\d+_\d+:", ln):
        m = re.search(r"Depth=(\d)", ln)
        depth = int(m.group(1)) if m else 0
        blocks.append([ln.split(":")[0], depth, 0, 0])
    elif ln.startswith("\t") and not ln.startswith(("\t.", "\t;")):
        op = ln.split()[0]
        ops.setdefault(depth, Counter())[op] += 1
        blocks[-1][2] += 1
        blocks[-1][3] += op.startswith("v_accvgpr")
print(name)
for d in sorted(ops):
    n = sum(ops[d].values())
    acc = sum(v for k, v in ops[d].items() if k.startswith("v_accvgpr"))
    f64 = sum(v for k, v in ops[d].items() if k.endswith(("_f64", "_f64_e32", "_f64_e64", "_f64_dpp")))
    print(f"depth {d}: {n:5d} instructions, {f64:5d} fp64, {acc:4d} AGPR moves")
print("blocks of at least", minblk, "instructions (label, depth, instructions, AGPR moves):")
for b in blocks:
    if b[2] >= minblk:
        print(f"  {b[0]:12s} {b[1]} {b[2]:5d} {b[3]:4d}")
