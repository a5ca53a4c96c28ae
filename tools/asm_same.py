#!/usr/bin/env python3
"""Do two hipcc -S listings hold the same code, kernel by kernel?

    python tools/asm_same.py parent/build/ntt_kernels.s build/ntt_kernels.s

Compares every `_Z` symbol of the two listings (`kernels()` of asm_hist.py:
kernels and the data symbols between them) as text, with what differs between
two builds of the same code taken out: assembler comments, the numbers of
basic-block and other local labels, and the hash in the `__hip_cuid_*` name.
Prints the symbols that differ or exist on one side only and exits non-zero
if there are any.  It knows no instruction names.
"""
import re
import sys

from asm_hist import kernels

_LABEL = re.compile(r'\.L[A-Za-z_]+[0-9_]*\d')
_CUID = re.compile(r'__hip_cuid_\w+')


def normalise(lines):
    """Instruction text of one symbol: comments and blank lines dropped,
    local labels renumbered in order of first appearance."""
    names, out = {}, []
    for line in lines:
        line = _CUID.sub('__hip_cuid', line.split(';', 1)[0]).strip()
        if line:
            out.append(_LABEL.sub(lambda m: names.setdefault(m.group(0), f'.L{len(names)}'), line))
    return out


def differing(path_a, path_b):
    """(number of symbols compared, sorted names that differ or are one-sided)"""
    a, b = kernels(path_a), kernels(path_b)
    bad = [n for n in sorted(set(a) | set(b)) if n not in a or n not in b or normalise(a[n]) != normalise(b[n])]
    return len(set(a) | set(b)), bad


def main():
    total, bad = differing(sys.argv[1], sys.argv[2])
    for name in bad:
        print(name)
    print(f"{total} symbols compared, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
