#!/usr/bin/env python3
"""One line per kernel of a device-only assembly listing: the SHA-256 of the kernel's text, and its name.

    hipcc --offload-arch=gfx950 <the Makefile's CXXFLAGS> --cuda-device-only -S device.hip -o device.s
    tools/kernel_bodies.py device.s > bodies.txt

Two listings whose lines are equal hold the same kernels, instruction for instruction: the way to show that a change to the sources (a refactor of
the templates, say) left the compiler's output alone.  A kernel's text is what stands between its label and its `.Lfunc_end` — the instructions and
the `.amdhsa_kernel` descriptor — with what differs between two compilations of the same code taken out: the kernel's own name, the numbers the
compiler gives its local labels (`.LBB<n>_<m>`, `.Ltmp<n>`, `.Lfunc_*<n>`: renumbered in order of appearance), comments and debug directives.  It
compares text and looks for nothing in it.

--map-forms rewrites the names of the listings from before the form words (k_shade<bool x 7>, k_path<bool x 4, Env...>) to the names they have
since (k_shade<FORM>, k_path<FORM, STATS, Env...>; loupiote_amd/csrc/kernel_forms.h), so that an old and a new listing can be joined by name."""
import argparse
import hashlib
import re
import sys

_LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
_LOCAL = re.compile(r"\.L(BB|tmp|func_begin|func_end|JTI|CPI)(\d+)")
_DEBUG = re.compile(r"^\.(loc|file|cfi_\w+|ident|addrsig\w*)\b")
_SHADE = re.compile(r"_ZN4lptd7k_shadeI((?:Lb[01]E){7})E")
_PATH = re.compile(r"_ZN4lptd6k_pathILb([01])ELb([01])ELb([01])ELb([01])E(\w*)DpT3_")   # the pack was the fifth template parameter and is the third


def map_forms(name):
    """the mangled name of a k_shade / k_path instantiation from before the form words, as it is spelled since"""
    def shade(m):
        bits = re.findall(r"Lb([01])E", m.group(1))   # GBUF, ENV, PUNCT, TRANS, EMIS, ESAMP, NMAP: bit i of the word
        return "_ZN4lptd7k_shadeILj%dEE" % sum(int(b) << i for i, b in enumerate(bits))

    def path(m):
        gbuf, stats, env, punct = (int(g) for g in m.groups()[:4])
        return "_ZN4lptd6k_pathILj%dELb%dE%sDpT1_" % (gbuf | env << 1 | punct << 2, stats, m.group(5))
    return _PATH.sub(path, _SHADE.sub(shade, name))


def _normalise(lines, name):
    local = {}

    def renumber(m):
        return ".L%s%d" % (m.group(1), local.setdefault((m.group(1), m.group(2)), len(local)))
    out = []
    for line in lines:
        line = line.split(";", 1)[0].replace(name, "@K").strip()
        if not line or _DEBUG.match(line):
            continue
        out.append(" ".join(_LOCAL.sub(renumber, line).split()))
    return "\n".join(out) + "\n"


def kernel_bodies(text):
    """[(name, sha256 of the normalised text)] for every kernel (a function with an .amdhsa_kernel descriptor) of the listing, in its order"""
    found, name, body = [], None, []
    for line in text.splitlines():
        m = _LABEL.match(line)
        if name is None:
            if m and not m.group(1).startswith(".L"):
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            if any(l.split() == [".amdhsa_kernel", name] for l in body):
                found.append((name, hashlib.sha256(_normalise(body, name).encode()).hexdigest()))
            name = None
            continue
        body.append(line)
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("listing", help="assembly from hipcc --cuda-device-only -S")
    ap.add_argument("--map-forms", action="store_true", help="rewrite k_shade<bools> / k_path<bools...> names to the form words")
    args = ap.parse_args()
    with open(args.listing, errors="replace") as f:
        bodies = kernel_bodies(f.read())
    for name, digest in sorted((map_forms(n) if args.map_forms else n, d) for n, d in bodies):
        print(digest, name)
    print("%d kernels" % len(bodies), file=sys.stderr)


if __name__ == "__main__":
    main()
