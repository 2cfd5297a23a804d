"""The set of kernel instantiations in libnlsolver_hip.so, pinned to tests/golden/kernel_set.txt.

Which instantiation a launch runs is picked on the host from run-time values (nlsg_dispatch.h); the
host stubs the compiler emits for exactly the instantiations the host code names are the record of
what those selections can reach. A change of the list is a change of the library's kernels: the
fixture is then re-recorded on purpose, never by accident."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nlsolver_amd", "libnlsolver_hip.so")
STUB = "__device_stub__"


def _symbol_tool():
    """A command that prints the library's full symbol table (.symtab: the stubs of static kernels are
    local symbols, which the dynamic table does not hold)."""
    rocm = [os.path.join(d, "llvm", "bin") for d in (os.environ.get("ROCM_PATH", ""), "/opt/rocm") if d]
    for name, args in (("nm", []), ("llvm-nm", []), ("llvm-readelf", ["--symbols", "--wide"])):
        for path in [shutil.which(name)] + [os.path.join(d, name) for d in rocm]:
            if path and os.path.exists(path):
                return [path] + args
    return None


def kernel_stubs():
    tool = _symbol_tool()
    assert tool is not None, "reading the library's symbol table needs nm, llvm-nm or llvm-readelf (binutils, or " \
                             "the ROCm tree's llvm/bin): none was found"
    out = subprocess.check_output(tool + [LIB], text=True)
    names = {line.split()[-1] for line in out.splitlines() if line.split() and STUB in line.split()[-1]}
    return sorted(names)


def test_library_holds_exactly_the_recorded_kernel_instantiations():
    with open(os.path.join(ROOT, "tests", "golden", "kernel_set.txt")) as f:
        recorded = f.read().split()
    assert recorded and recorded == sorted(set(recorded)), "the fixture is a sorted list of distinct names"
    built = kernel_stubs()
    added = sorted(set(built) - set(recorded))
    missing = sorted(set(recorded) - set(built))
    print(f"{len(set(built) & set(recorded))} of {len(recorded)} recorded kernels in the library")
    for name in added:
        print("added:  ", name)
    for name in missing:
        print("missing:", name)
    assert not added and not missing, f"{len(added)} kernels added, {len(missing)} missing (names above)"
    assert len(built) == len(recorded)


def test_recorded_kernel_families_have_their_sizes():
    """The fixture itself: how many instantiations each dispatched family has."""
    with open(os.path.join(ROOT, "tests", "golden", "kernel_set.txt")) as f:
        recorded = f.read().split()
    sizes = {"pso_move_kernel": 64, "de_turn_kernel": 52, "de_generation_kernel": 52, "pso_batch_kernel": 40,
             "bfgs_search_kernel": 40, "bfgs_init_kernel": 40, "sann_anneal_kernel": 32,
             "pso_move_groups_kernel": 32, "de_batch_kernel": 20, "nm_solve_kernel": 16,
             "lm_wide_fd_eval_kernel": 16, "nmpso_solve_wide_kernel": 12, "bfgs_resident_kernel": 10,
             "nm_solve_driver_kernel": 7, "lm_wide_chol_step_kernel": 6}
    for family, n in sizes.items():
        assert sum(f"{STUB}{family}I" in name for name in recorded) == n, family
