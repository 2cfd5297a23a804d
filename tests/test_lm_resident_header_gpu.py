"""The drop-in header's LevenbergMarquardt on a device::CurveModel<double> (exponential decay) with
device::lm_driver_mode() = turns and = resident, and with NLSG_LM_DRIVER=resident in the environment: theta
and the status, printed as hexadecimal floats, are the same text in all three runs. The program is written
and compiled here, with the host compiler."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nlsolver_mi/nlsolver.h"

namespace dev = nlsolver::device;

// header_lm_resident turns | resident | env      (env: the mode NLSG_LM_DRIVER gives, or the default)
int main(int argc, char **argv) {
  if (argc != 2) return 2;
  const size_t m = 64, n = 3;
  std::vector<double> t(m), y(m), x = {1.7, 0.9, 0.45};
  for (size_t i = 0; i < m; i++) {
    t[i] = 4.0 * static_cast<double>(i) / 63.0;
    y[i] = 2.0 * std::exp(-0.7 * t[i]) + 0.5 + 0.01 * std::sin(7.0 * static_cast<double>(i));
  }
  try {
    if (!std::strcmp(argv[1], "turns")) dev::lm_driver_mode() = dev::lm_driver::turns;
    else if (!std::strcmp(argv[1], "resident")) dev::lm_driver_mode() = dev::lm_driver::resident;
    else if (std::strcmp(argv[1], "env")) return 2;
    std::fprintf(stderr, "mode=%d library_has_resident=%d\n",
                 dev::lm_driver_mode() == dev::lm_driver::resident ? 1 : 0,
                 dev::api::get().has_lm_resident() ? 1 : 0);
    dev::CurveModel<double> model(m, n, 1, t, y,
                                  "const double e = det_exp(-th(1) * t(0));\n"
                                  "r = y - (th(0) * e + th(2));\n"
                                  "J(0) = -e;  J(1) = th(0) * t(0) * e;  J(2) = -1.0;");
    auto solver = nlsolver::LevenbergMarquardt<dev::CurveModel<double>, double>(model);
    auto [fcalls, iters, f, g, h] = solver.minimize(x).get_summary();
    std::printf("fcalls=%zu iters=%zu gcalls=%zu hcalls=%zu f=%a x=%a,%a,%a\n", fcalls, iters, g, h, f, x[0], x[1],
                x[2]);
  } catch (const nlsolver::device_error &e) {
    std::fprintf(stderr, "device_error: %s\n", e.what());
    return 3;
  }
  return 0;
}
"""


def test_header_drivers_agree(tmp_path):
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from nlsolver_amd import _capi
    src, exe = str(tmp_path / "header_lm_resident.cpp"), str(tmp_path / "header_lm_resident")
    with open(src, "w") as fh:
        fh.write(PROGRAM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off",
                           "-I" + os.path.join(ROOT, "include"), src, "-o", exe, "-ldl"])
    base = {k: v for k, v in os.environ.items() if k != "NLSG_LM_DRIVER"}
    base["NLSG_LIBRARY"] = _capi.LIB_PATH

    def run(mode, **extra):
        p = subprocess.run([exe, mode], env=dict(base, **extra), text=True, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr
        return p.stdout, p.stderr

    turns, log_t = run("turns")
    resident, log_r = run("resident")
    by_env, log_e = run("env", NLSG_LM_DRIVER="resident")
    assert "mode=0" in log_t and "mode=1 library_has_resident=1" in log_r and "mode=1 library_has_resident=1" in log_e
    assert turns.startswith("fcalls=") and " iters=" in turns
    assert int(turns.split("iters=")[1].split()[0]) >= 2
    assert resident == turns
    assert by_env == turns
