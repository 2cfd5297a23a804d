#!/usr/bin/env python3
"""Regenerate tests/golden/nm_hostile.json: the UNMODIFIED reference's NelderMead (oracle/_ref/ref_driver
nm-hostile) on the hostile objective families of tests/_hostile.py, for the even-n runs that
tests/_direct_cases.golden_runs() names. Per run: function calls, iterations, f and x as hexfloat.

Only works where the reference is present; the JSON written here is committed (data only).
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
DRIVER = os.path.join(ROOT, "oracle", "_ref", "ref_driver")

from tests import _direct_cases as Cs  # noqa: E402


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    if not os.path.exists(DRIVER):
        sys.exit("reference driver not built (is the reference present?)")
    runs = {}
    for name, r in Cs.golden_runs():
        b = Cs.batch_by_name(name)
        row = b.rows[r]
        args = [b.n, row.family, row.a, row.b, b.step, b.max_iter, b.eps, b.no_change, b.restarts,
                row.x0, row.dx, int(b.bounded), b.upper, b.lower, int(b.minimize)]
        out = subprocess.check_output([DRIVER, "nm-hostile", *map(repr, args)], text=True)
        runs[f"{name}/{r}"] = dict(json.loads(out), args=[repr(a) for a in args])
    with open(os.path.join(HERE, "nm_hostile.json"), "w") as fh:
        json.dump({"driver": "nm-hostile D family a b step max_iter eps no_change restarts x0 x0_step "
                             "bounded upper lower minimize", "runs": runs}, fh, separators=(",", ":"))
        fh.write("\n")
    print(len(runs), "runs")


if __name__ == "__main__":
    main()
