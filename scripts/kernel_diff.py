"""Per-kernel comparison of two builds of the library (no GPU needed):  python scripts/kernel_diff.py OLD NEW

OLD / NEW: two libggd_raster.so, or two directories of `-S` listings (python -m gaussian_gan_decoder_amd.build --save-temps).
Prints, per kernel, `same` or `DIFF` for the instruction stream (comments, directives, addresses and encodings stripped, `.LBB<n>_`
labels normalised) and VGPR / SGPR / LDS / scratch / kernarg of both builds side by side; then one summary line and the kernels
whose kernarg size changed.  A kernel of OLD whose name is gone is compared with the kernel of NEW whose template arguments are
OLD's with `false` arguments added (a feature flag that became a defaulted template parameter), or, with
`--dropped KERNEL:I,J` (0-based positions, repeatable), OLD's without the listed arguments.  Exit status 1 on any DIFF, resource
change or unmatched kernel."""
from __future__ import annotations

import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, code_objects, demangle, parse_metadata, short  # noqa: E402


def streams_of(text: str, syms, objdump: bool) -> dict:
    """{kernel symbol: [instruction, ...]} of a disassembly (llvm-objdump -d) or a compiler listing (-S)"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:$", line) if objdump else re.match(r"([A-Za-z_][\w$.]*):", line)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in syms else None
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", re.split(r"//|;", line)[0]).strip()
        if cur is None or not line or (line.startswith(".") and not line.endswith(":")):
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        else:
            cur.append(" ".join(line.split()))
    for ins in out.values():   # padding behind the last instruction
        while ins and ins[-1].split()[0] in ("s_nop", "s_code_end"):
            ins.pop()
    return out


def load(path: str) -> dict:
    """{short demangled name: (figures, instruction stream)}"""
    res, ins = {}, {}
    with tempfile.TemporaryDirectory() as td:
        for f in (sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else code_objects(path, td)):
            one = {}
            if os.path.isdir(path):
                text = open(f).read()
                parse_metadata(text, one)
            else:
                parse_metadata(subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], capture_output=True, text=True).stdout, one)
                text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f], capture_output=True, text=True, check=True).stdout
            res.update(one)
            ins.update(streams_of(text, set(one), not os.path.isdir(path)))
    syms = list(res)
    return {short(n): (res[s], ins.get(s, [])) for n, s in zip(demangle(syms), syms)}


def targs(name: str):
    return name.split("<")[0], ([a.strip() for a in name[name.index("<") + 1:name.rindex(">")].split(",")] if "<" in name else [])


def padded(old, new) -> bool:   # new = old with `false` arguments inserted
    i = 0
    for a in new:
        if i < len(old) and a == old[i]:
            i += 1
        elif a != "false":
            return False
    return i == len(old)


if __name__ == "__main__":
    dropped = {}   # kernel -> template argument positions that NEW no longer has
    while "--dropped" in sys.argv:
        k, pos = sys.argv.pop(sys.argv.index("--dropped") + 1).split(":")
        sys.argv.remove("--dropped")
        dropped[k] = [int(i) for i in pos.split(",")]
    old, new = load(sys.argv[1]), load(sys.argv[2])
    left = [n for n in new if n not in old]
    same = bad = 0
    kernarg = []
    for name in sorted(old):
        base, args = targs(name)
        args = [a for i, a in enumerate(args) if i not in dropped.get(base, ())]
        cands = [name] if name in new else [n for n in left if targs(n)[0] == base and padded(args, targs(n)[1])]
        if len(cands) != 1:
            print(f"{'UNMATCHED':9s} {name}  (candidates: {cands})")
            bad += 1
            continue
        if cands[0] in left:
            left.remove(cands[0])
        (ro, io), (rn, inn) = old[name], new[cands[0]]
        ok = io == inn and len(io) > 0
        res_ok = all(ro.get(k, 0) == rn.get(k, 0) for k in ("vgpr", "agpr", "sgpr", "lds", "scratch", "vgpr_spill", "sgpr_spill"))
        same += ok and res_ok
        bad += not (ok and res_ok)
        if ro.get("kernarg") != rn.get("kernarg"):
            kernarg.append(f"  {cands[0]}: kernarg {ro.get('kernarg')} -> {rn.get('kernarg')} B")
        fig = "  ".join(f"{k} {ro.get(k, 0)}|{rn.get(k, 0)}" for k in ("vgpr", "sgpr", "lds", "scratch", "kernarg"))
        print(f"{'same' if ok else 'DIFF':4s} {'' if res_ok else 'RES '}{len(io):6d} instr  {fig}  {name}" + ("" if cands[0] == name else f" -> {cands[0]}"))
    for n in left:
        print(f"{'NEW ONLY':9s} {n}")
    print(f"{same} of {len(old)} kernels identical (instruction stream, VGPR, SGPR, LDS, scratch); {bad} differ or unmatched; "
          f"{len(left)} only in the new build; {len(kernarg)} kernarg sizes changed")
    print("\n".join(kernarg))
    sys.exit(1 if bad or left else 0)
