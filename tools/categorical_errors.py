#!/usr/bin/env python3
"""Collects the MAXERR lines of tests/test_gpu_categorical.py from a kept `pytest -s` output into
profiles/<run>_categorical_errors.json: per group of cases (the envelope's shapes, the degenerate class sets, K = 2
against the oracle's logistic density, scaled coefficients) the largest lp and gradient error as a fraction of the
1e-10 bars, with the shape it occurred at, and every parity case's pair.

usage: tools/categorical_errors.py --run r31a --log categorical.log"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"MAXERR categorical\[(?:(?P<group>[a-z]+)(?P<scale>[0-9.e+]*)-)?(?P<dims>[0-9-]+)\] lp=(?P<lp>\S+) grad=(?P<g>\S+)")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--run", required=True)
    p.add_argument("--log", required=True)
    a = p.parse_args()
    with open(a.log) as fh:
        text = fh.read()
    largest, cases = {}, []
    for m in LINE.finditer(text):
        group = m.group("group") or "envelope"
        dims = [int(v) for v in m.group("dims").split("-")]
        rec = largest.setdefault(group, {"cases": 0, "lp": None, "grad": None})
        rec["cases"] += 1
        cases.append({"group": group + (m.group("scale") or ""), "dims": dims, "lp": float(m.group("lp")), "grad": float(m.group("g"))})
        for key, v in (("lp", float(m.group("lp"))), ("grad", float(m.group("g")))):
            if rec[key] is None or v > rec[key]["value"]:
                rec[key] = {"value": float(f"{v:.4g}"), "dims": dims, **({"scale": m.group("scale")} if m.group("scale") else {})}
    passed = re.search(r"\d+ (passed|failed)[^\n]*", text)
    out = {"tool": "tools/categorical_errors.py",
           "unit": "the 1e-10 bars of tests/test_gpu_categorical.py (lp over max(|lp|, 1); gradient over "
                   "max(|g_j|, 1e-3 (max |g| + 1))); <= 1 passes",
           "dims": "envelope, degenerate classes and scaled coefficients: K, d, n, C; logistic: d, n, C",
           "pytest_summary": passed.group(0).strip("= ") if passed else None,
           "largest_over_bar": max((r[k]["value"] for r in largest.values() for k in ("lp", "grad") if r[k]), default=None),
           "largest_errors_over_bar": dict(sorted(largest.items())),
           "cases": cases}
    path = os.path.join(ROOT, "profiles", f"{a.run}_categorical_errors.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"groups": {k: v["cases"] for k, v in largest.items()}, "largest": out["largest_over_bar"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
