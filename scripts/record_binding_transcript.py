#!/usr/bin/env python3
"""Records tests/golden/binding_transcript.json.gz (JSON, gzipped for its repetition: `zcat` shows it):
for every case of tests/_binding_transcript.py the C calls the Python binding makes on a fake library,
what it returns and raises, and the package's public surface. No device is needed. Run it at the commit whose behaviour is the yardstick (the file in the
tree was recorded at the parent of the commit that gave the engine classes one base);
tests/test_binding_transcript_cpu.py only ever reads the file.

    python3 scripts/record_binding_transcript.py [--out FILE]"""
import argparse
import gzip
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nlsolver_amd import _capi  # noqa: E402
from tests import _binding_transcript as T  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_transcript.json.gz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    rec = {"commit": subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip(),
           "surface": T.surface(), "cases": {}}
    for case in T.cases():
        fake = T.FakeLibrary(case.missing, case.fail)
        _capi._lib = fake
        try:
            rec["cases"][case.id] = T.record(case, fake)
        finally:
            _capi._lib = None
    text = json.dumps(rec, indent=0, sort_keys=True) + "\n"
    with open(args.out, "wb") as f:  # (mtime 0: the same record gives the same file)
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:
            z.write(text.encode())
    print(f"{len(rec['cases'])} cases, {os.path.getsize(args.out)} bytes -> {args.out}")


if __name__ == "__main__":
    main()
