#!/usr/bin/env python3
"""Compare the instruction streams of the kernels two builds have in common, from the gfx950 code objects of their objects.

A kernel is paired with the OLD kernel of the same name and template arguments (kernels in an anonymous namespace by their own
names).  Where there is none, a kernel of the NEW object whose last template argument is `false` is paired with the OLD kernel of
the same name without that argument (bh_walk_rows_kernel<false> with bh_walk_rows_kernel, bh_walk_lane_kernel<true, false> with bh_walk_lane_kernel<true>), so
that a kernel that has gained a compile-time switch can be checked to be, in its `false` form, the kernel it was.  Addresses,
encodings, comments and the padding behind a function are dropped; branch offsets are relative, so identical code compares equal
wherever it was placed.

A kernel whose template arguments changed otherwise is paired by hand: --pair 'nbody::k<false>=nbody::k<false, 2, false>' (old = new,
names as this tool prints them).

    python3 tools/isa_compare.py OLD.o NEW.o [--only SUBSTRING] [--pair OLD=NEW ...]   # exit code 1 if a pair differs or a kernel has no partner

--mask-registers: a pair whose streams differ, but are equal once every register number — scalar, vector or accumulator, single or a
range — is replaced by a placeholder, is printed as `same instructions, registers differ` and does not count as differing.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_hazards import LLVM, code_object   # noqa: E402


def kernels(obj, workdir):
    """{demangled function name: [instruction lines]} of the object's code object."""
    co = code_object(obj, workdir)
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "-C", "--no-show-raw-insn", "--no-leading-addr", co], check=True,
                         capture_output=True, text=True).stdout
    out, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^<(.+)>:$", ln.strip())
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        code = ln.split("//")[0].strip()
        if cur is not None and code:
            out[cur].append(" ".join(code.split()))
    for ins in out.values():                                     # the padding up to the next function's alignment
        while ins and ins[-1] in ("s_nop 0", "..."):
            ins.pop()
    return out


def masked(ins):
    """the instruction lines with register numbers replaced: v14 -> vN, s[10:11] -> s[N]"""
    return [re.sub(r"\b([vsa])(?:\d+|\[\d+:\d+\])", lambda m: m.group(1) + ("N" if m.group(0)[1] != "[" else "[N]"), ln) for ln in ins]


def base(name):
    """(name without return type and parameters, template arguments or None)"""
    name = name.replace("(anonymous namespace)::", "").split("(")[0]   # (nbody::(anonymous namespace)::k<..>(..) is nbody::k<..>)
    name = name.split(" ")[-1] if not name.endswith(">") else name[name.rfind(" ", 0, name.find("<")) + 1:]
    if name.endswith(">"):
        i = name.find("<")
        return name[:i], [a.strip() for a in name[i + 1:-1].split(",")]
    return name, None


def key_new(name):
    b, args = base(name)
    if args is None or args[-1] != "false":
        return None
    return b + ("<" + ", ".join(args[:-1]) + ">" if len(args) > 1 else "")


def key_old(name):
    b, args = base(name)
    return b + ("<" + ", ".join(args) + ">" if args else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--only", default="", help="compare the kernels whose name holds this")
    ap.add_argument("--pair", action="append", default=[], metavar="OLD=NEW", help="the NEW kernel of this name is the OLD kernel of that name")
    ap.add_argument("--mask-registers", action="store_true", help="a pair that differs in register numbers alone does not count as differing")
    a = ap.parse_args()
    renamed = {new: old for old, new in (p.split("=", 1) for p in a.pair)}
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new:
        old = {key_old(k): v for k, v in kernels(a.old, t_old).items() if a.only in k}
        new = {}
        for k, v in kernels(a.new, t_new).items():
            if a.only not in k:
                continue
            if key_old(k) in renamed:
                new[renamed[key_old(k)]] = v
            elif key_old(k) in old or base(k)[1] is None:        # the same name on both sides: that pair
                new[key_old(k)] = v
            elif key_new(k) is not None:
                new[key_new(k)] = v
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print(f"{k}: only in the {'old' if k in old else 'new'} object")
            bad += 1
            continue
        verdict = "identical" if old[k] == new[k] else "DIFFERENT"
        if verdict == "DIFFERENT" and a.mask_registers and masked(old[k]) == masked(new[k]):
            verdict = "same instructions, registers differ"
        print(f"{k}: {len(old[k])} / {len(new[k])} instructions, {verdict}")
        bad += verdict == "DIFFERENT"
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
