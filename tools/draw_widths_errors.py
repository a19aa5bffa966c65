#!/usr/bin/env python3
"""Collects the MAXERR lines of tests/test_gpu_draw_widths.py from a kept `pytest -s` output into
profiles/<run>_draw_widths_errors.json: per sweep and family the largest error of every checked quantity in
units of its bar (with the KF and d it occurred at), the same split into the KF the older test files already
ran (1, 2, 4, 5, 25, 32) and the 26 they did not, and every KF whose error is more than OUTLIER x the median
over the 32.

usage: tools/draw_widths_errors.py --run r24a --log profiles/r24a_draw_widths_gpu.log"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"MAXERR widths (?P<sweep>\w+) family=(?P<family>\w+) kf=(?P<kf>\d+): (?P<rest>.*) \(units of the bar\)")
ITEM = re.compile(r"(\w+)=(\S+)@d=(\d+)")
OLD_KF = (1, 2, 4, 5, 25, 32)
OUTLIER = 5.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--run", required=True)
    p.add_argument("--log", required=True)
    a = p.parse_args()
    with open(a.log) as fh:
        text = fh.read()
    vals = {}                                        # (sweep, family, key) -> {kf: (value, d)}
    for m in LINE.finditer(text):
        for key, v, d in ITEM.findall(m.group("rest")):
            vals.setdefault((m.group("sweep"), m.group("family"), key), {})[int(m.group("kf"))] = (float(v), int(d))
    largest, outliers = {}, []
    for (sweep, family, key), by_kf in sorted(vals.items()):
        def top(kfs):
            kf = max(kfs, key=lambda k: by_kf[k][0])
            return {"value": by_kf[kf][0], "kf": kf, "d": by_kf[kf][1]}
        old = [k for k in by_kf if k in OLD_KF]
        new = [k for k in by_kf if k not in OLD_KF]
        med = statistics.median(v for v, _ in by_kf.values())
        largest[f"{sweep}.{family}.{key}"] = {"n_kf": len(by_kf), "all": top(by_kf), "kf_run_before": top(old),
                                             "kf_first_run_here": top(new), "median_over_kf": med}
        for kf, (v, d) in sorted(by_kf.items()):
            if med > 0 and v > OUTLIER * med:
                outliers.append({"quantity": f"{sweep}.{family}.{key}", "kf": kf, "d": d, "value": v, "median_over_kf": med})
    passed = re.search(r"(\d+) passed", text)
    rec = {"tool": "tools/draw_widths_errors.py", "source": os.path.relpath(os.path.abspath(a.log), ROOT),
           "unit": "each quantity's own bar (tests/test_gpu_draw_widths.py); <= 1 passes",
           "pytest_summary": passed.group(0) if passed else None, "kf_run_before": list(OLD_KF),
           "outlier_rule": f"value > {OUTLIER} x the median over the 32 KF", "outliers": outliers,
           "largest_errors_over_bar": largest}
    out = os.path.join(ROOT, "profiles", f"{a.run}_draw_widths_errors.json")
    with open(out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"quantities": len(largest), "outliers": len(outliers),
                      "largest": max((v["all"]["value"] for v in largest.values()), default=None)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
