#!/usr/bin/env python3
"""Compares the gfx950 kernels of two builds (no GPU needed): for every kernel symbol the sequence of instruction
encodings of a plain llvm-objdump -d, and the register / scratch / LDS figures of tools/kernel_regs.py.  Addresses
and file offsets are not compared, so a kernel may sit in another object, or at another place in it.
  python tools/kernel_isa_diff.py --a FILE [FILE ...] --b FILE [FILE ...] [--out REPORT] [--rename-b OLD=NEW ...]
FILE: object files or libipdamg.so.  Exit status 1 when a kernel is missing on one side or differs.
--rename-b: a kernel of b whose demangled name contains OLD is paired with the kernel of a that has NEW there (a type
that became a template instantiation changes the mangled name and nothing else); kernels of b that stay unpaired
after the renames are listed as ONLY IN b and counted apart with --allow-new.
--distinct: a template that several units instantiate has one body per unit; compare the DISTINCT bodies (and figures)
of each kernel instead of the sorted lists, so that a second copy that went away is no difference, and report the
copies per side (x2 -> x1) and how many kernels lost or gained copies."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_regs import LLVM, code_objects, kernel_rows  # noqa: E402


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernel_code(paths, kernels):
    """mangled kernel symbol -> its bodies (a template that two units instantiate has one in each), sorted; a body
    is a list of instruction encodings"""
    code = {}
    for path in paths:
        for co in code_objects(path):
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(co)
                f.flush()
                txt = subprocess.run([LLVM + "/llvm-objdump", "-d", f.name], capture_output=True, text=True).stdout
            sym = None
            for line in txt.split("\n"):
                m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
                if m:
                    # (labels inside a kernel carry no symbol of their own in these objects: a new symbol is a new function)
                    sym = m.group(1)
                    if sym in kernels:
                        code.setdefault(sym, []).append([])
                    continue
                m = re.search(r"// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)$", line)
                if m and sym in code:
                    code[sym][-1].append(m.group(1).strip())
    for bodies in code.values():   # the filler behind a function's last instruction (s_nop 0, s_code_end: up to the
        for b in bodies:           # next function's alignment, or to the end of the section) is not its code
            while b and b[-1] in ("BF800000", "BF9F0000"):
                b.pop()
    return {s: sorted(b) for s, b in code.items()}


def kernel_symbols(paths):
    syms = set()
    for path in paths:
        for co in code_objects(path):
            with tempfile.NamedTemporaryFile(suffix=".co") as f:
                f.write(co)
                f.flush()
                txt = subprocess.run([LLVM + "/llvm-readelf", "--notes", f.name], capture_output=True, text=True).stdout
            syms.update(re.findall(r"\.name:\s+(\S+)", txt))
    return syms


def figures(paths):
    rows = {}
    for dem, fig in kernel_rows(paths):
        rows.setdefault(dem, []).append(fig)
    return {d: sorted(f) for d, f in rows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", nargs="+", required=True)
    ap.add_argument("--b", nargs="+", required=True)
    ap.add_argument("--out")
    ap.add_argument("--rename-b", nargs="*", default=[], metavar="OLD=NEW")
    ap.add_argument("--allow-new", action="store_true", help="kernels only in b are listed but are no failure")
    ap.add_argument("--distinct", action="store_true", help="compare each kernel's distinct bodies, report the copies")
    args = ap.parse_args()
    ka, kb = kernel_symbols(args.a), kernel_symbols(args.b)
    ca, cb = kernel_code(args.a, ka), kernel_code(args.b, kb)
    ra, rb = figures(args.a), figures(args.b)
    names = demangle(sorted(ka | kb))
    # kernels are paired by demangled name, b's after the renames; everything below is keyed by a's name
    renames = [r.split("=", 1) for r in args.rename_b]

    def renamed(dem):
        for old, new in renames:
            dem = dem.replace(old, new)
        return dem

    short = lambda dem: dem.replace("(anonymous namespace)", "{anonymous}").split("(")[0]
    key_b = {renamed(names[s]): s for s in kb}
    key_a = {names[s]: s for s in ka}
    rb = {short(renamed(names[s])): rb.get(short(names[s])) for s in kb}
    ca = {names[s]: c for s, c in ca.items()}
    cb = {renamed(names[s]): c for s, c in cb.items()}
    ka, kb = set(key_a), set(key_b)
    names = {k: k for k in ka | kb}
    lines, bad, new, recount = [], 0, 0, 0

    def uniq(seq):   # sorted distinct entries (bodies are lists)
        out = []
        for x in sorted(seq or []):
            if not out or out[-1] != x:
                out.append(x)
        return out

    same = (lambda x, y: uniq(x) == uniq(y)) if args.distinct else (lambda x, y: x == y)
    for sym in sorted(ka | kb, key=lambda s: names[s]):
        dem = short(names[sym])
        if sym in ka and sym in kb and (sym not in ca or sym not in cb):
            lines.append("%-72s NO CODE FOUND IN %s" % (dem[-72:], "a" if sym not in ca else "b"))
            bad += 1
            continue
        if sym not in ka or sym not in kb:
            lines.append("%-72s ONLY IN %s" % (dem[-72:], "a" if sym in ka else "b"))
            if sym in kb and args.allow_new:
                new += 1
            else:
                bad += 1
            continue
        na, nb = [len(b) for b in ca[sym]], [len(b) for b in cb[sym]]
        if same(ca[sym], cb[sym]) and min(na) > 0 and same(ra.get(dem), rb.get(dem)):
            if len(na) != len(nb):   # (only with --distinct)
                recount += 1
                copies = "  (x%d -> x%d, %d distinct -> %d)" % (len(na), len(nb), len(uniq(ca[sym])), len(uniq(cb[sym])))
            else:
                copies = "  (x%d)" % len(na) if len(na) > 1 else ""
            lines.append("%-72s identical  %6d instructions  %s%s" % (dem[-72:], na[0], ra[dem][0], copies))
        else:
            bad += 1
            lines.append("%-72s DIFFERS    %s -> %s instructions (%+d)" % (dem[-72:], na, nb, sum(nb) - sum(na)))
            lines.append("    a: %s" % "; ".join(ra.get(dem, [])))
            lines.append("    b: %s" % "; ".join(rb.get(dem, [])))
    head = ["a: " + " ".join(args.a), "b: " + " ".join(args.b),
            "renames of b: " + (" ".join(args.rename_b) or "none"),
            "%d kernels in a, %d in b, %d in both; %d missing or different; %d only in b and allowed" %
            (len(ka), len(kb), len(ka & kb), bad, new)]
    if args.distinct:
        head.append("distinct bodies compared: %d bodies in a, %d in b; %d kernels with another number of copies" %
                    (sum(len(c) for c in ca.values()), sum(len(c) for c in cb.values()), recount))
    head.append("")
    text = "\n".join(head + lines) + "\n"
    if args.out:
        open(args.out, "w").write(text)
    sys.stdout.write(text if not args.out else "\n".join(head) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
