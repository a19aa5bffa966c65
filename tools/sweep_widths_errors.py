#!/usr/bin/env python3
"""Collects the MAXERR lines of tests/test_gpu_sweep_widths.py from a kept `pytest -s` output into
profiles/<run>_sweep_widths_errors.json: per sweep kernel and family the largest lp and gradient error in
units of the 1e-10 bar, with the width and the chain batch it occurred at, and the number of batches seen.

usage: tools/sweep_widths_errors.py --run r25a --log widths.log"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"MAXERR widths\[(?P<family>[a-z]+)-(?P<d>\d+)-B(?P<B>\d+)-(?P<kind>\w+)\] "
                  r"lp_rel=(?P<lp>\S+) grad_over_scale=(?P<g>\S+)")
BAR = 1e-10


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--run", required=True)
    p.add_argument("--log", required=True)
    a = p.parse_args()
    with open(a.log) as fh:
        text = fh.read()
    largest, widths = {}, set()
    for m in LINE.finditer(text):
        d, B = int(m.group("d")), int(m.group("B"))
        widths.add(d)
        rec = largest.setdefault(f"{m.group('kind')}.{m.group('family')}", {"batches": 0, "lp": None, "grad": None})
        rec["batches"] += 1
        for key, v in (("lp", float(m.group("lp")) / BAR), ("grad", float(m.group("g")) / BAR)):
            if rec[key] is None or v > rec[key]["value"]:
                rec[key] = {"value": float(f"{v:.4g}"), "d": d, "B": B}
    passed = re.search(r"\d+ passed[^\n]*", text)
    out = {"tool": "tools/sweep_widths_errors.py",
           "unit": "the 1e-10 bars of tests/test_gpu_sweep_widths.py (lp over max(|lp|, 1); gradient over "
                   "max(|g_j|, 1e-3 (max |g| + 1))); <= 1 passes",
           "pytest_summary": passed.group(0).strip("= ") if passed else None, "widths": len(widths),
           "largest_over_bar": max((r[k]["value"] for r in largest.values() for k in ("lp", "grad")), default=None),
           "largest_errors_over_bar": dict(sorted(largest.items()))}
    path = os.path.join(ROOT, "profiles", f"{a.run}_sweep_widths_errors.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"kernel_families": len(largest), "widths": len(widths), "largest": out["largest_over_bar"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
