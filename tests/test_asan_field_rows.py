"""Sanitizer run of the field sweep's row selection (no GPU, nothing loaded into Python).

``make -C plate_inverse_problem_amd/csrc asan-field`` builds ``csrc/field_rows_asan.cpp`` + ``plan.cpp`` +
``symbolic.cpp`` with g++ ``-fsanitize=address,undefined`` (no recovery, runtimes linked statically): a stand-alone
program that passes ``pfr::field_rows`` -- the validation and permutation ``pfr_field_sweep`` runs before it launches
anything -- the selections a caller can pass, each list in a heap block of exactly its size.  The accepted ones must
map every row through the permutation; an index outside [0, n), an empty or a null list must be refused with the
message the C ABI returns."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plate_inverse_problem_amd", "csrc")
EXE = os.path.join(CSRC, "..", "_lib", "asan", "field_rows_asan")


@pytest.fixture(scope="module")
def exe():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asan-field"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.exists(EXE)
    return EXE


@pytest.mark.parametrize("n", [4, 97, 19353])
def test_field_rows_under_asan_ubsan(exe, n):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(n)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}
    n_desc = 2 * ((n + 1) // 2)
    for name, count in (("all", n), ("one", 1), ("descending", n_desc), ("prefix", 33 if n > 33 else n // 2)):
        assert got[name][0] == "ok" and int(got[name][1]) == count, (name, got[name])
    for name in ("index_n", "index_minus_one", "index_int_min", "empty_perm"):
        assert got[name][0] == "refused" and "outside" in got[name], (name, got[name])
    for name in ("no_rows", "negative_count", "null_list"):
        assert got[name][0] == "refused" and "least" in got[name], (name, got[name])
