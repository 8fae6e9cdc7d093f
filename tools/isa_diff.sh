#!/bin/bash
export DEMI_EXPERIMENT=1     # the library reads its experiment / diagnostic variables only with this set (csrc/knobs.hpp)
# tools/isa_diff.sh [<git rev>]  - which gfx950 kernels does the working tree compile to different instructions than <rev> (HEAD)?
# No GPU needed.  The generic kernels of libdemi_gpu.so are compared symbol by symbol (device-only compilation of demi_gpu.hip,
# disassembled), the kernels specialised for raft5 - the narrow table, the wide one, which alone gets the recording and
# carried-generator modules compiled, and the one with akka-raft's field sets (DEMI_MODEL_PAYLOADS) - by the .text of their code objects (demi_specialize_check under DEMI_JIT_DUMP).  A change that is meant to leave a hot kernel alone should show that kernel as SAME here before it goes to
# the GPU; scratch under gpurun_out/isa_diff (git-ignored).
set -e
REV=${1:-HEAD}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
G=$ROOT/gpurun_out/isa_diff
LLVM=/opt/rocm/lib/llvm/bin
rm -rf "$G"; mkdir -p "$G"
git -C "$ROOT" worktree add -f "$G/wt" "$REV" -q
trap 'git -C "$ROOT" worktree remove --force "$G/wt"' EXIT
for t in A B; do
  r=$([ $t = A ] && echo "$G/wt" || echo "$ROOT")
  ( cd "$r" && python -c "import __graft_entry__ as G; G._write_jit_sources()" &&
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -c demi_amd/csrc/demi_gpu.hip -o "$G/dev$t.o" &&
    $LLVM/clang-offload-bundler --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$G/dev$t.o" --output="$G/co$t.o" &&
    $LLVM/llvm-objdump -d --no-show-raw-insn "$G/co$t.o" > "$G/dis$t.txt" ) &
done
wait
( cd "$G/wt" && python -c "import __graft_entry__ as G; G.build()" )
( cd "$ROOT" && python -c "import __graft_entry__ as G; G.build()" )
cat > "$G/dump.py" <<'PY'
import sys, os
root, out = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); os.chdir(root)
os.environ["DEMI_JIT_DUMP"] = out
os.environ["DEMI_SPECIALIZE_CHECK_TESTS"] = "1"     # (the workgroup-per-test modules too, where the tree has them)
os.environ["DEMI_SPECIALIZE_CHECK_ROUND"] = "1"     # (and the wildcard round's module)
from demi_amd import _native, model as M
assert _native.__file__.startswith(root)
_native.specialize_check(M.raft_model(5).to_struct())
os.environ["DEMI_JIT_DUMP"] = out + "_wide"           # (the table tools/jit_stats.py --wide looks at)
_native.specialize_check(M.raft_model(5, term0=1000, loglen0=300).to_struct())
os.environ["DEMI_JIT_DUMP"] = out + "_fields"         # (a DEMI_MODEL_PAYLOADS table: the kernels that read payload areas)
_native.specialize_check(M.raft_model(5, log_cap=8, real_fields=True).to_struct())
PY
python "$G/dump.py" "$G/wt" "$G/jitA"; python "$G/dump.py" "$ROOT" "$G/jitB"
python - "$G" <<'PY'
import re, hashlib, shutil, sys, os, subprocess
G = sys.argv[1]
# What is compared is the instructions.  Three things differ between two builds of the same code and are normalised: the
# symbol's name inside branch-target annotations, the pc-relative displacement of a call into another function (the s_add_u32
# behind s_getpc_b64: it moves when any function in between changes size) and the alignment padding behind the last instruction.
def per(fn):
    d, cur = {}, None
    for l in open(fn):
        m = re.match(r'^[0-9a-f]+ <(.*)>:', l)
        if m: cur = m.group(1); d[cur] = []; continue
        if cur and l.strip(): d[cur].append(re.sub(r'<[^>]*>', '', re.sub(r'//.*', '', l)).strip())
    for v in d.values():
        while v and (v[-1].startswith('s_nop') or v[-1] == '...'): v.pop()
        for i in range(1, len(v)):
            if v[i - 1].startswith('s_getpc_b64') and v[i].startswith('s_add_u32'): v[i] = re.sub(r'0x[0-9a-f]+$', 'REL', v[i])
    return {k: (hashlib.md5("\n".join(v).encode()).hexdigest()[:8], len(v)) for k, v in d.items() if k.startswith('_Z')}
# Kernels are matched by their demangled names, K1's template arguments spelled <REC, FIFO, CARRY, variant> whichever way the
# tree declares them: up to seven bools (REC, FIFO, CARRY, then REBIN, MULTI, SPREAD, TESTS, of which at most one is set), or
# three bools and a K1Variant.
VARIANTS = ["K1_PLAIN", "K1_REBIN", "K1_MULTI", "K1_SPREAD", "K1_TESTS"]
def k1_args(m):
    p = [x.strip() for x in m.group(1).split(",")]
    if p[-1] in ("true", "false"):
        p += ["false"] * (7 - len(p))
        p = p[:3] + [VARIANTS[1 + p[3:].index("true")] if "true" in p[3:] else VARIANTS[0]]
    else:
        p[3] = VARIANTS[int(re.sub(r'\(.*\)', '', p[3]))] if re.sub(r'\(.*\)', '', p[3]).isdigit() else p[3].split("::")[-1]
    return 'k1_random_explore<' + ", ".join(p) + '>'
filt = shutil.which('llvm-cxxfilt') or shutil.which('c++filt') or '/opt/rocm/lib/llvm/bin/llvm-cxxfilt'
def named(d):
    names = list(d)
    dem = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for k, n in zip(names, dem):
        n = re.sub(r'k1_random_explore<([^>]*)>', k1_args, n)
        out[re.sub(r'K1ArgsOf<[^>]*>::type', 'K1ArgsOf::type', n)] = d[k]
    return out
a, b = named(per(G + '/disA.txt')), named(per(G + '/disB.txt'))
for k in sorted(set(a) | set(b)):
    st = "SAME" if a.get(k) == b.get(k) else "NEW " if k not in a else "GONE" if k not in b else "DIFF"
    print("generic     %s %-110s %s -> %s" % (st, k[:110], a.get(k, ("-", 0))[1], b.get(k, ("-", 0))[1]))
for table, suffix in (("raft5", ""), ("raft5 wide", "_wide"), ("raft5 fields", "_fields")):
  for k in range(64):          # (every module either tree dumped: demi_gpu.hip JK_COUNT)
    h = []
    for t in "AB":
        p = "%s/jit%s%s.%d" % (G, t, suffix, k)
        if not os.path.exists(p): h.append(None); continue
        subprocess.check_call(["/opt/rocm/lib/llvm/bin/llvm-objcopy", "-O", "binary", "--only-section=.text", p, p + ".text"])
        h.append(hashlib.md5(open(p + ".text", "rb").read()).hexdigest()[:8])
    if h[0] or h[1]: print("specialised %s kernel %d (%s) %s -> %s" % ("SAME" if h[0] == h[1] else "NEW " if not h[0] else "GONE" if not h[1] else "DIFF", k, table, h[0], h[1]))
PY
