#!/usr/bin/env python3
"""Records tests/golden/engine_doors.json: for every case of tests/_engine_doors.py the code a rejected
C-ABI call returns with the text of nlsg_last_error, and the values of the pure size functions. No call
of the table reaches a device, so the record is the same on every machine. Run it on a library built at
the commit whose behaviour is the yardstick and name that checkout, so that its hash goes into the file
(the file in the tree was recorded at the parent of the commit that gave the engine files one set of
front doors); tests/test_engine_doors_cpu.py only ever reads the file.

    NLSG_LIBRARY=<checkout>/nlsolver_amd/libnlsolver_hip.so \\
        python3 scripts/record_engine_doors.py --checkout <checkout> [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nlsolver_amd import _capi  # noqa: E402
from tests import _engine_doors as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkout", default=ROOT, help="the git checkout the library was built from")
    ap.add_argument("--out", default=D.GOLDEN)
    args = ap.parse_args()
    rec = {"commit": subprocess.check_output(["git", "-C", args.checkout, "rev-parse", "HEAD"], text=True).strip()}
    rec.update(D.replay(_capi.lib()))
    with open(args.out, "w") as f:
        f.write(json.dumps(rec, indent=0, sort_keys=True) + "\n")
    print(f"{len(rec['cases'])} cases, {len(rec['pure'])} values, {os.path.getsize(args.out)} bytes "
          f"-> {args.out} ({_capi.LIB_PATH} at {rec['commit'][:12]})")


if __name__ == "__main__":
    main()
