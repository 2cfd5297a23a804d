#!/usr/bin/env python3
"""Regenerate tests/golden/tinyqr_hostile.json: the UNMODIFIED reference's tinyqr (oracle/_ref/ref_driver
tinyqr-hex) on the systems of tests/_tinyqr_cases.py. Per base case (n <= 40, p <= 12): the inputs, Q and R
of qr_decomposition (default tol 1e-8), back_solve's beta on them, lm's beta at the default tol and at the
case's tol, all as hexfloat with nan / inf spelled out. Per wide member (regenerated from the case file, not
stored): the betas, and hashes of Q and R that read every NaN as the one quiet NaN.

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

from tests import _tinyqr_cases as Cs  # noqa: E402


def run(case):
    text = " ".join(Cs.hexes(case.X)) + "\n" + " ".join(Cs.hexes(case.y)) + "\n"
    out = subprocess.check_output([DRIVER, "tinyqr-hex", str(case.n), str(case.p), float(case.tol).hex()],
                                  input=text, text=True)
    return json.loads(out)


def main():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
    if not os.path.exists(DRIVER):
        sys.exit("reference driver not built (is the reference present?)")
    base, wide = {}, {}
    for c in Cs.base_cases():
        base[c.name] = dict(run(c), kind=c.kind, X=Cs.hexes(c.X), y=Cs.hexes(c.y))
    for w in Cs.WIDTHS:
        for c in Cs.wide_cases(w):
            r = run(c)
            wide[c.name] = dict(n=r["n"], p=r["p"], tol=r["tol"], Q_fnv=r["Q_fnv"], R_fnv=r["R_fnv"],
                                X_fnv=str(Cs.fnv(c.X)), y_fnv=str(Cs.fnv(c.y)),
                                **{f"{k}_fnv": str(Cs.fnv(Cs.unhex(r[k]))) for k in ("beta", "beta_tol", "beta_tol1e-8")})
    with open(os.path.join(HERE, "tinyqr_hostile.json"), "w") as fh:
        json.dump({"driver": "tinyqr-hex n p tol < X (column-major n x p) y", "base": base, "wide": wide}, fh,
                  separators=(",", ":"))
        fh.write("\n")
    print(len(base), "base cases,", len(wide), "wide members")


if __name__ == "__main__":
    main()
