"""dev tool: do two builds of the library hold the same device code?  For a refactor that must not change a kernel.
    python tools/compare_code_objects.py OLD_OBJ_DIR NEW_OBJ_DIR [--map OLD=NEW ...] [--pooled]

Both directories are kmers_amd/csrc/_obj of a `python -m kmers_amd.build --force`.  For every object in both, the gfx950 code object
is unbundled and disassembled; each function's instructions (addresses dropped, encodings kept; the pc-relative offset of a call resolved to its target) and each kernel's
resource line (<src>.usage.txt) are compared by DEMANGLED name, after the --map substitutions (plain text, applied to the old
names: a renamed type, e.g. --map 'kmx::SinkHist,=kmx::SinkHistTable<kmx::HashLex, false>,').  Prints one line per object and
exits 1 if anything differs.

--pooled: for a refactor that moves kernels between source files.  The functions and usage lines of ALL objects of a build are pooled
and compared by demangled name alone; a name several objects define (an anonymous-namespace kernel of a shared header) counts as the
set of its bodies.  Prints one line for the pool and one per name that differs.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _demangle(names: list[str]) -> list[str]:
    if not names:
        return []
    r = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    return r.stdout.splitlines()


def _functions(obj: str, tmp: str) -> dict[str, list[str]]:
    """demangled function name -> its instructions (encodings and operands, no addresses, no comments)"""
    fatbin = os.path.join(tmp, os.path.basename(obj) + ".fatbin")
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fatbin], check=True)
    if os.path.getsize(fatbin) == 0:   # (host code only)
        open(co, "wb").close()
        return {}
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}",
                    f"--input={fatbin}", f"--output={co}"], check=True)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    starts = sorted((int(a, 16), n) for a, n in re.findall(r"^([0-9a-f]+) <(.+)>:$", dis, re.M))

    def symbolic(addr: int) -> str:
        i = max((j for j, (a, _) in enumerate(starts) if a <= addr), default=None)
        return f"<{starts[i][1]}+{addr - starts[i][0]:#x}>" if i is not None else f"{addr:#x}"

    funcs: dict[str, list[str]] = {}
    cur = None
    pc = None   # s_getpc_b64: (register, address after it) -- the s_add_u32 behind it adds a pc-relative offset
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        if cur is None or not ln.strip():
            continue
        # "<instruction>  // <address>: <encoding words> [<branch target>]" -> instruction and encoding
        ins, _, com = ln.partition("//")
        addr, _, rest = com.partition(":")
        enc = rest.split("<")[0].split()
        ops = ins.split()
        if ops[:1] == ["s_getpc_b64"]:
            pc = (ops[1].split(":")[0].replace("s[", "s"), int(addr, 16) + 4)
        elif pc and ops[:1] == ["s_add_u32"] and ops[1] == pc[0] + "," and ops[-1].startswith("0x"):
            # a call or a constant reached pc-relatively: compare the target, not the distance (the layout of the object may move)
            ops[-1] = symbolic((pc[1] + int(ops[-1], 16) - (1 << 32 if int(ops[-1], 16) >= 1 << 31 else 0)) & ((1 << 64) - 1))
            enc = enc[:1]
            pc = None
        cur.append(" ".join(ops + enc))
    for body in funcs.values():   # (the padding up to the next function depends on the layout, not on the code)
        while body and (body[-1] == "..." or body[-1].startswith("s_nop 0 ")):
            body.pop()
    return dict(zip(_demangle(list(funcs)), funcs.values()))


def _usage(path: str) -> dict[str, str]:
    if not os.path.exists(path):
        return {}
    rows = [ln.rstrip("\n").split(" | ", 1) for ln in open(path) if ln.strip()]
    return dict(zip(_demangle([r[0] for r in rows]), [r[1] if len(r) > 1 else "" for r in rows]))


def _mapped(d: dict, maps: list[tuple[str, str]]) -> dict:
    out = {}
    for name, v in d.items():
        for a, b in maps:
            name = name.replace(a, b)
        out[name] = v
    return out


def _pool(d: str, tmp: str, maps: list[tuple[str, str]]) -> tuple[dict[str, set], dict[str, set]]:
    """every object of a build: demangled name -> the set of its bodies, demangled name -> the set of its usage lines"""
    funcs: dict[str, set] = {}
    usage: dict[str, set] = {}
    os.makedirs(tmp, exist_ok=True)
    for f in sorted(os.listdir(d)):
        if f.endswith(".o"):
            for n, body in _mapped(_functions(os.path.join(d, f), tmp), maps).items():
                funcs.setdefault(n, set()).add(tuple(body))
            for n, u in _mapped(_usage(os.path.join(d, f[:-2] + ".usage.txt")), maps).items():
                usage.setdefault(n, set()).add(u)
    return funcs, usage


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], help="OLD=NEW text substitution on the old build's demangled names")
    ap.add_argument("--pooled", action="store_true", help="compare by name over all objects of each build, not object by object")
    a = ap.parse_args()
    maps = [tuple(m.split("=", 1)) for m in a.map]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        if a.pooled:
            (fo, uo), (fn, un) = _pool(a.old, os.path.join(tmp, "o"), maps), _pool(a.new, os.path.join(tmp, "n"), [])
            diff = [n for n in sorted(set(fo) | set(fn)) if fo.get(n) != fn.get(n)]
            udiff = [n for n in sorted(set(uo) | set(un)) if uo.get(n) != un.get(n)]
            print(f"{'pooled':34s} {len(fn):4d} functions  {'DIFFERENT' if diff or udiff else 'same code'}")
            for kind, names, old, new in (("code ", diff, fo, fn), ("usage", udiff, uo, un)):
                for n in names:
                    print(f"    {kind} {'missing in new' if n not in new else 'missing in old' if n not in old else 'differs'}: {n[:160]}")
            return 1 if diff or udiff else 0
        for f in sorted(os.listdir(a.old)):
            if not f.endswith(".o") or not os.path.exists(os.path.join(a.new, f)):
                continue
            po, pn = os.path.join(a.old, f), os.path.join(a.new, f)
            os.makedirs(os.path.join(tmp, "o"), exist_ok=True)
            os.makedirs(os.path.join(tmp, "n"), exist_ok=True)
            fo = _mapped(_functions(po, os.path.join(tmp, "o")), maps)
            fn = _functions(pn, os.path.join(tmp, "n"))
            same_bytes = open(os.path.join(tmp, "o", f + ".co"), "rb").read() == open(os.path.join(tmp, "n", f + ".co"), "rb").read()
            uo = _mapped(_usage(po[:-2] + ".usage.txt"), maps)
            un = _usage(pn[:-2] + ".usage.txt")
            diff = [n for n in sorted(set(fo) | set(fn)) if fo.get(n) != fn.get(n)]
            udiff = [n for n in sorted(set(uo) | set(un)) if uo.get(n) != un.get(n)]
            ok = not diff and not udiff
            bad += not ok
            print(f"{f:34s} {len(fn):4d} functions  {'identical bytes' if same_bytes else 'same code' if ok else 'DIFFERENT'}")
            for n in diff[:10]:
                print(f"    code  {'missing in new' if n not in fn else 'missing in old' if n not in fo else 'differs'}: {n[:160]}")
            for n in udiff[:10]:
                print(f"    usage {'missing in new' if n not in un else 'missing in old' if n not in uo else 'differs'}: {n[:160]}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
