#!/usr/bin/env python3
"""Records tests/golden/engine_cached_bytes.json: what the device pool parks after each create /
destroy case of tests/_engine_lifecycle.py, the codes and parked bytes of creates whose run-time
compilation fails, and the "parameters not set" texts. Run it on a gfx950 device at the commit whose
behaviour is the yardstick (the file in the tree was recorded at the parent of the commit that
added it); tests/test_engine_lifecycle_gpu.py only ever reads the file.

    python3 scripts/record_engine_cached_bytes.py [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nlsolver_amd import _capi  # noqa: E402
from tests import _engine_lifecycle as L  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=L.GOLDEN)
    args = ap.parse_args()
    lib = _capi.lib()
    rec = {"cycle": {}, "rtc_failure": {}, "messages": {}}
    for name in L.ENGINES:
        L.emptied(lib)
        first, second = L.cycle(lib, name), L.cycle(lib, name)
        assert first == second, (name, first, second)
        rec["cycle"][name] = first
    for name in L.RTC_FAILURES:
        L.emptied(lib)
        code, parked = L.failed_create(lib, name)
        rec["rtc_failure"][name] = {"code": code, "bytes": parked}
    L.emptied(lib)
    rec["nm_phase"] = L.nm_phase_cycle(lib)
    L.emptied(lib)
    rec["tinyqr_lm"], rec["tinyqr_qr"] = L.tinyqr_calls(lib)
    for kind in L.PARAM_KINDS:
        rec["messages"][kind] = L.param_messages(lib, kind)
    L.emptied(lib)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
