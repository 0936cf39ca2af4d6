#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, function by function.

    asm_diff.py <dir_a> <dir_b>

Each directory holds the device assembly of the translation units of one build, one `.s` per unit:

    hipcc <FLAGS of build.py> -x hip --offload-device-only -S csrc/<unit> -o <dir>/<unit>.s

A refactor that moves kernels between units or touches host code only must leave every function's body, its `.amdhsa_kernel` block and
its metadata entry (registers, scratch, LDS, kernarg layout) byte-equal, and every symbol defined exactly once over all units.  The
per-unit function index in local labels (`.LBB<n>_<m>`, `.LJTI<n>_<m>`, `.Lfunc_begin<n>`, `.Lfunc_end<n>`, `BB<n>_<m>` in loop comments) is normalised away; which
unit a function lives in is not compared.  Prints the differences; exit status 1 if there is any.
"""
import glob
import os
import re
import sys

_INDEX = re.compile(r"\.(LBB|LJTI|Lfunc_begin|Lfunc_end)\d+")
_COMMENT = re.compile(r"\bBB\d+_(\d+)")      # the same index in the loop comments, whose column moves with the label's width
_TYPE = re.compile(r"^\t\.type\t(\S+),@function")


def _functions(lines):
    """symbol -> text from its `.type` line to its `.size` line plus the resource comments behind it"""
    out, sym, buf, closed = {}, None, [], False
    for ln in lines:
        m = _TYPE.match(ln)
        if m or (closed and not ln.lstrip().startswith(";")):
            if sym:
                out.setdefault(sym, []).append("\n".join(buf))
            sym, buf, closed = (m.group(1), [], False) if m else (None, [], False)
        if sym:
            buf.append(re.sub(r"\s+;", " ;", _COMMENT.sub(r"BB#_\1", _INDEX.sub(r".\1#", ln))))
            if ln.startswith("\t.size\t" + sym + ","):
                closed = True
    if sym:
        out.setdefault(sym, []).append("\n".join(buf))
    return out


def _metadata(lines):
    """kernel symbol -> its entry of amdhsa.kernels"""
    out, entry, inside = {}, [], False
    def close():
        names = [e.split(":", 1)[1].strip() for e in entry if e.strip().startswith(".name:")]
        if names:
            out[names[0]] = "\n".join(entry)
    for ln in lines:
        if ln.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and (ln.startswith("  - ") or not ln.startswith(" ")):
            close()
            entry = [ln]
            inside = ln.startswith(" ")
        elif inside:
            entry.append(ln)
    return out


def load(directory):
    funcs, meta = {}, {}
    files = sorted(glob.glob(os.path.join(directory, "*.s")))
    if not files:
        sys.exit(f"no .s files in {directory}")
    for path in files:
        lines = open(path).read().split("\n")
        unit = os.path.basename(path)
        for sym, texts in _functions(lines).items():
            funcs.setdefault(sym, []).extend((unit, t) for t in texts)
        for sym, text in _metadata(lines).items():
            meta.setdefault(sym, []).append((unit, text))
    return funcs, meta


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    (fa, ma), (fb, mb) = load(sys.argv[1]), load(sys.argv[2])
    bad = 0
    for tag, funcs in (("a", fa), ("b", fb)):
        for sym, defs in sorted(funcs.items()):
            if len(defs) > 1:
                bad += 1
                print(f"defined {len(defs)} times in {tag}: {sym} ({', '.join(u for u, _ in defs)})")
    for sym in sorted(set(fa) - set(fb)):
        bad += 1
        print(f"only in a: {sym} ({fa[sym][0][0]})")
    for sym in sorted(set(fb) - set(fa)):
        bad += 1
        print(f"only in b: {sym} ({fb[sym][0][0]})")
    kernels = 0
    for sym in sorted(set(fa) & set(fb)):
        kernels += ".amdhsa_kernel" in fa[sym][0][1]
        what = []
        if fa[sym][0][1] != fb[sym][0][1]:
            what.append("code / .amdhsa_kernel block")
        if [t for _, t in ma.get(sym, [])][:1] != [t for _, t in mb.get(sym, [])][:1]:
            what.append("metadata")
        if what:
            bad += 1
            print(f"differs ({', '.join(what)}): {sym} ({fa[sym][0][0]} | {fb[sym][0][0]})")
    print(f"{len(fa)} functions in a, {len(fb)} in b, {kernels} kernels in both, {bad} difference(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
