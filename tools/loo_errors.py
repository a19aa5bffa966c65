#!/usr/bin/env python3
"""Collects the MAXERR lines of tests/test_gpu_loo.py (one pytest run in a child process) into
profiles/<run>_loo_errors.json: per case the largest row and total errors in units of the 1e-10 bars,
the largest khat error and the case's khat bar, and the largest of each over all cases.

usage: tools/loo_errors.py --run r18a [--log FILE]   (--log: parse a kept pytest -s output instead)"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"MAXERR loo\[(?P<case>[^\]]+)\] rows (?P<rows>\S+)(?: totals (?P<totals>\S+))?"
                  r"(?: \(units of the 1e-10 bars?\))?(?: khat (?P<khat>\S+) bar (?P<bar>\S+))?")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--run", default="r18a")
    p.add_argument("--log", default=None)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.log:
        with open(a.log) as fh:
            text = fh.read()
        rc = 0
    else:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_loo.py"), "-q", "-s",
                            "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=ROOT)
        text, rc = r.stdout, r.returncode
    cases = {}
    for m in LINE.finditer(text):
        rec = {k: float(v) for k, v in m.groupdict().items() if k != "case" and v is not None}
        cases.setdefault(m.group("case"), {}).update(rec)
    worst = {k: max((c[k] for c in cases.values() if k in c), default=None) for k in ("rows", "totals", "khat", "bar")}
    rec = {"tool": "tools/loo_errors.py", "pytest_exit_code": rc, "n_cases": len(cases),
           "units": {"rows": "1e-10 max(1, max |ll|)", "totals": "1e-10 max(1, sum |term|)", "khat": "absolute",
                     "bar": "khat bar of the case: max(1e-10, 1000 x the float64 restatement's error)"},
           "largest": worst, "cases": cases}
    out = a.out or os.path.join(ROOT, "profiles", f"{a.run}_loo_errors.json")
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: rec[k] for k in ("pytest_exit_code", "n_cases", "largest")}))
    return rc


if __name__ == "__main__":
    sys.exit(main())
