#!/usr/bin/env python
"""Census of the never-skipped narrow regions of a compiled K1, and of how often they are empty.  No GPU needed.

  python tools/k1_empty_census.py /tmp/img.0 [-v]      static: a dumped K1 code object (DEMI_JIT_DUMP=<path> -> <path>.0)
  python tools/k1_empty_census.py --emu [N]            dynamic: the census build of K1 on the wave64 emulator (tests/emu)

Static.  Inside the main loop (the span of the longest backward branch, as tools/k1_loop_size.py finds it) every instruction
that NARROWS the exec mask (s_and_saveexec / s_andn2_saveexec / s_or_saveexec, s_and / s_andn2 into exec) and has no
s_cbranch_execz / s_cbranch_execnz before the first vector instruction behind it: the wave issues what follows whether or not
a lane is left.  Per such region - it ends where exec is written next, or at a branch - the vector instructions (VALU, LDS,
vector memory) and the 32 x 32 multiplies among them.  -v lists every region with its address.

Dynamic.  K1 compiled with DEMI_K1_CENSUS (k1_random_explore.hpp K1_SITE: off by default, emulator only - it prints) runs
config 2 (apps.raft5_config2: raft5, the 50-event trace) over N schedules (default 4096) in normal lane order, interpreter and
compiled kernel; per source site the wave iterations in which NO lane entered it, of the iterations the wave was live."""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTOR = ("v_", "ds_", "global_", "flat_", "buffer_", "scratch_")
MUL32 = ("v_mad_u64_u32", "v_mad_i64_i32", "v_mul_lo_u32", "v_mul_hi_u32", "v_mul_lo_i32", "v_mul_hi_i32")
SITES = ["until == 0 (checkpoint / message limit)", "flush: some lane has a batch to append", "timer queue not empty at the step",
         "nextInt: modulo path (bound no power of two)", "nextInt: rejected draw", "is_rep: delivered timer is parked",
         "timersToResend re-enter (n_resend != 0)", "queue capacity reached (any site)", "pending capacity reached (any append)",
         "cancel: timer may be in messagesToSend", "cancel: directory entry is TD_MANY (scan)", "quiescence branch"]


def parse(path):
    dis = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", path], capture_output=True, text=True).stdout.splitlines()
    ins = []
    for l in dis:
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", l)
        if m:
            ins.append((int(m.group(3), 16), m.group(1), m.group(2)))
    return ins


def main_loop(ins):
    index = {a: i for i, (a, _, _) in enumerate(ins)}
    best = None
    for i, (a, op, args) in enumerate(ins):
        if op.startswith("s_cbranch") or op == "s_branch":
            try:
                off = int(args.split()[-1])
            except ValueError:
                continue
            if off >= 32768:
                off -= 65536
            tgt = a + 4 + 4 * off
            if tgt < a and tgt in index and (best is None or i - index[tgt] > best[1] - best[0]):
                best = (index[tgt], i)
    return best


def writes_exec(op, args):
    return "saveexec" in op or (op.startswith("s_") and args.split(",")[0].strip() == "exec")


def narrows(op, args):
    if "saveexec" in op:
        return True
    return op in ("s_and_b64", "s_andn2_b64") and args.split(",")[0].strip() == "exec"


def static_census(path, verbose):
    ins = parse(path)
    lo, hi = main_loop(ins)
    body = ins[lo:hi + 1]
    kinds = collections.Counter(op.split("_")[0] for _, op, _ in body if op != "s_nop")
    n_branch = sum(1 for _, op, _ in body if op in ("s_cbranch_execz", "s_cbranch_execnz"))
    regions = []
    for i, (a, op, args) in enumerate(body):
        if not narrows(op, args):
            continue
        j, guarded = i + 1, False
        while j < len(body) and not body[j][1].startswith(VECTOR):
            o, g = body[j][1], body[j][2]
            if o in ("s_cbranch_execz", "s_cbranch_execnz"):
                guarded = True
                break
            if writes_exec(o, g) or o.startswith("s_cbranch") or o == "s_branch":
                break
            j += 1
        if guarded:
            continue
        vec, mul = 0, 0
        j = i + 1
        while j < len(body):
            o, g = body[j][1], body[j][2]
            if writes_exec(o, g) or o.startswith("s_cbranch") or o == "s_branch":
                break
            if o.startswith(VECTOR):
                vec += 1
                mul += o in MUL32
            j += 1
        regions.append((a, op, vec, mul))
    total = sum(1 for _, op, _ in body if op != "s_nop")
    vecs = sum(1 for _, op, _ in body if op.startswith(VECTOR))
    print("%s: main loop %d instructions %s, %d execz / execnz branches" % (path, total, dict(kinds), n_branch))
    print("exec narrowings with no skip branch behind them: %d, holding %d vector instructions (%.1f %% of the loop's %d), %d of them 32 x 32 multiplies"
          % (len(regions), sum(r[2] for r in regions), 100.0 * sum(r[2] for r in regions) / max(vecs, 1), vecs, sum(r[3] for r in regions)))
    hist = collections.Counter(r[2] for r in regions)
    print("vector instructions per region: count   " + "  ".join("%d: %d" % (k, hist[k]) for k in sorted(hist)))
    print("regions of 5 or more: %d;  of 3 or more, or with a multiply: %d" % (sum(1 for r in regions if r[2] >= 5), sum(1 for r in regions if r[2] >= 3 or r[3])))
    if verbose:
        for a, op, vec, mul in regions:
            print("  %08x  %-22s %2d vector%s" % (a, op, vec, ", %d multiplies" % mul if mul else ""))


EMU_DRIVER = r"""
import os, sys
sys.path.insert(0, %(root)r)
from tests.emu import build
b = build.build()
os.environ["DEMI_NO_TORCH"] = "1"
os.environ["DEMI_HIPRTC_LIB"] = b["hiprtc"]
from demi_amd import _native
from demi_amd.apps import raft5_config2
_native.LIB_PATH = b["lib"]
model, events, lim = raft5_config2()
ctx = _native.Context(0)
ctx.model_load(model.to_struct())
ctx.model_specialize()
ctx.trace_load(events)
ctx.random_explore(%(n)d, lim, seed_base=0x5EED0000)
ctx.close()
"""


def emu_census(n):
    env = dict(os.environ, DEMI_EXPERIMENT="1", DEMI_JIT_DEFINES="DEMI_K1_CENSUS=1", W64_THREADS="1")
    env.pop("W64_LANE_ORDER", None)
    out = subprocess.run([sys.executable, "-c", EMU_DRIVER % {"root": ROOT, "n": n}], cwd=ROOT, env=env, capture_output=True, text=True)
    if out.returncode:
        sys.exit(out.stdout[-2000:] + out.stderr[-4000:])
    iters, empty, lanes = 0, collections.Counter(), collections.Counter()
    for l in out.stdout.splitlines():
        f = l.split()
        if len(f) == 5 and f[0] == "K1CENSUS":
            s = int(f[1])
            if s == 0:
                iters += int(f[4])
            empty[s] += int(f[2])
            lanes[s] += int(f[3])
    if not iters:
        sys.exit("no census lines: was the kernel compiled with DEMI_K1_CENSUS?\n" + out.stdout[-2000:] + out.stderr[-2000:])
    print("config 2, %d schedules, compiled K1 on the emulator: %d live wave iterations" % (n, iters))
    print("| site | iterations with no lane in it | lanes in it per iteration |")
    print("|---|---|---|")
    for s, name in enumerate(SITES):
        print("| %s | %.1f %% | %.2f |" % (name, 100.0 * empty[s] / iters, lanes[s] / iters))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--emu":
        emu_census(int(a[1]) if len(a) > 1 else 4096)
    else:
        for p in [x for x in a if x != "-v"]:
            static_census(p, "-v" in a)
