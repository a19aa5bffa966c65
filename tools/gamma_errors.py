#!/usr/bin/env python3
"""Collects the MAXERR lines of tests/test_gpu_gamma.py from a kept `pytest -s` output, and the shape terms' largest
ratios from tests/test_host_gamma.py (run here with STARK_GAMMA_ERRORS_OUT set), into profiles/<run>_gamma_errors.json:
per group of cases (outlier data, precise data, scaled coefficients) the largest lp and gradient error as a fraction
of the 1e-10 bars, with the shape it occurred at.

usage: tools/gamma_errors.py --run r29a --log gamma.log [--host host.json]"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"MAXERR gamma\[(?P<group>[a-z]+)(?P<scale>[0-9.e+]*)-(?P<n>\d+)-(?P<d>\d+)-(?P<C>\d+)\] lp=(?P<lp>\S+) grad=(?P<g>\S+)")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--run", required=True)
    p.add_argument("--log", required=True)
    p.add_argument("--host", default=None, help="the JSON tests/test_host_gamma.py wrote (STARK_GAMMA_ERRORS_OUT)")
    a = p.parse_args()
    with open(a.log) as fh:
        text = fh.read()
    largest = {}
    for m in LINE.finditer(text):
        rec = largest.setdefault(m.group("group"), {"cases": 0, "lp": None, "grad": None})
        rec["cases"] += 1
        shape = [int(m.group("n")), int(m.group("d")), int(m.group("C"))]
        for key, v in (("lp", float(m.group("lp"))), ("grad", float(m.group("g")))):
            if rec[key] is None or v > rec[key]["value"]:
                rec[key] = {"value": float(f"{v:.4g}"), "n_d_C": shape, **({"scale": m.group("scale")} if m.group("scale") else {})}
    passed = re.search(r"\d+ (passed|failed)[^\n]*", text)
    out = {"tool": "tools/gamma_errors.py",
           "unit": "the 1e-10 bars of tests/test_gpu_gamma.py (lp over max(|lp|, 1); gradient over "
                   "max(|g_j|, 1e-3 (max |g| + 1))); <= 1 passes",
           "pytest_summary": passed.group(0).strip("= ") if passed else None,
           "largest_over_bar": max((r[k]["value"] for r in largest.values() for k in ("lp", "grad") if r[k]), default=None),
           "largest_errors_over_bar": dict(sorted(largest.items()))}
    if a.host:
        with open(a.host) as fh:
            out["shape_terms_over_1e-13_bars"] = json.load(fh)
    path = os.path.join(ROOT, "profiles", f"{a.run}_gamma_errors.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"groups": {k: v["cases"] for k, v in largest.items()}, "largest": out["largest_over_bar"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
