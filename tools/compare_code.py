#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libhbvx.so: kernel set, resource rows and instructions.

    python tools/compare_code.py old.so new.so

Each kernel's disassembly (llvm-objdump -d --no-show-raw-insn, address comments and the padding after
it stripped) is compared as text: branch targets are relative, so a kernel's instructions do not depend
on where it lies.  Exit status 1 when the new build has a kernel the old one lacks, or a kernel of both
changed its resources or instructions; kernels may go."""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import LLVM, code_objects, kernel_table  # noqa: E402


def disassembly(lib: str) -> dict[str, str]:
    """symbol -> position-free instruction text of every kernel in lib"""
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for co in code_objects(lib, td):
            text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co],
                                  check=True, capture_output=True, text=True).stdout
            for m in re.finditer(r"^[0-9a-f]+ <([^>]+)>:\n(.*?)(?=\n\n|\Z)", text, re.S | re.M):
                body = [re.sub(r"\s*//.*$", "", ln).strip() for ln in m.group(2).splitlines()]
                out[m.group(1)] = "\n".join(ln for ln in body if ln and ln != "...")   # ("...": padding)
    return out


def main(old: str, new: str) -> int:
    rows = [{r["symbol"]: r for r in kernel_table(lib)} for lib in (old, new)]
    code = [disassembly(lib) for lib in (old, new)]
    gone, added = sorted(rows[0].keys() - rows[1].keys()), sorted(rows[1].keys() - rows[0].keys())
    keep = sorted(rows[0].keys() & rows[1].keys())
    rows_diff = [s for s in keep if rows[0][s] != rows[1][s]]
    code_diff = [s for s in keep if code[0].get(s) != code[1].get(s) or s not in code[0]]
    print(f"{len(rows[0])} -> {len(rows[1])} kernels: {len(gone)} gone, {len(added)} new, "
          f"{len(rows_diff)} with changed resources, {len(code_diff)} with changed instructions")
    for s in gone:
        print("  gone:", rows[0][s]["name"])
    for tag, names in (("new", added), ("resources", rows_diff), ("instructions", code_diff)):
        for s in names:
            print(f"  {tag}:", (rows[1] if tag == "new" else rows[0])[s]["name"])
    return 1 if added or rows_diff or code_diff else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
