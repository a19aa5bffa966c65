#!/usr/bin/env python3
"""Instruction counts of k_sweep_cat's sub-tile loop, read from a build's sweep_cat.o (needs no GPU).

    python tools/categorical_isa.py stark_amd/_lib/obj/sweep_cat.o [--shapes 3x100,5x64,9x32] [--out FILE]

The gfx950 code object is taken out of the object file as tools/codeobj_compare.py does and disassembled with
llvm-objdump.  For the instantiation k_sweep_cat<K - 1, 4 ceil(d / 16)> of every shape K x d, the instructions from the
first to the last v_mfma of the kernel -- one trip of the sub-tile loop: forward, residual, backward -- are counted:
the MFMAs, the other vector instructions (v_*; of those the v_accvgpr_* copies between the two register halves), the
LDS reads (ds_read*).  A lane holds 4 rows of a chain per sub-tile, so vector instructions per (row, chain) element are
the count / 4, and per class that / G.  One JSON object on stdout and to --out: what `tools/categorical_cost.py --isa`
records.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from codeobj_compare import LLVM, code_object, run  # noqa: E402


def loops(obj):
    """{(G, KF): [instruction mnemonics from the first to the last v_mfma]} of every k_sweep_cat in obj."""
    with tempfile.TemporaryDirectory() as tmp:
        dis = run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", code_object(obj, tmp))
    out, key, text = {}, None, []

    def close():
        if key is not None:
            idx = [i for i, t in enumerate(text) if t.startswith("v_mfma")]
            out[key] = text[idx[0]:idx[-1] + 1] if idx else []

    for line in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            close()
            k = re.search(r"k_sweep_catILi(\d+)ELi(\d+)E", m.group(1))
            key, text = ((int(k.group(1)), int(k.group(2))) if k else None), []
        elif line.startswith("\t") and key is not None:
            text.append(line.strip().split()[0])
    close()
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("obj")
    p.add_argument("--shapes", default="3x100,5x64,9x32", help="K x d, comma separated")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    per = loops(a.obj)
    res = {"how": "tools/categorical_isa.py: llvm-objdump of the build's sweep_cat.o, first to last v_mfma of the kernel"}
    for spec in a.shapes.split(","):
        K, d = (int(v) for v in spec.split("x"))
        G, KF = K - 1, 4 * ((d + 15) // 16)
        t = per[(G, KF)]
        valu = sum(1 for i in t if i.startswith("v_") and not i.startswith("v_mfma"))
        res[f"K={K},d={d}"] = {"kernel": f"k_sweep_cat<{G}, {KF}>", "mfma_per_subtile": sum(1 for i in t if i.startswith("v_mfma")),
                              "valu_per_subtile": valu, "of_which_accvgpr_moves": sum(1 for i in t if i.startswith("v_accvgpr")),
                              "lds_reads_per_subtile": sum(1 for i in t if i.startswith("ds_read")),
                              "valu_per_row_chain_element": valu / 4, "valu_per_element_per_class": valu / 4 / G}
    text = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
