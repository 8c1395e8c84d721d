"""Sanitizer run of the field-loss sweep's row and weight validation (no GPU, nothing loaded into Python).

``make -C plate_inverse_problem_amd/csrc asan-field-loss`` builds ``csrc/field_loss_rows_asan.cpp`` + ``plan.cpp`` +
``symbolic.cpp`` with g++ ``-fsanitize=address,undefined`` (no recovery, runtimes linked statically): a stand-alone
program that passes ``pfr::field_loss_rows`` -- what ``pfr_field_loss_sweep`` runs before it launches anything -- the
lists a caller can pass, each in a heap block of exactly its size.  The accepted ones must map every row through the
permutation; a repeated row (the adjoint seed is a scatter), a row outside [0, n), an empty list, a weight that is
negative or not finite, all weights zero and weights beside a cotangent must be refused with the message the C ABI
returns, and leave no partial selection behind."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plate_inverse_problem_amd", "csrc")
EXE = os.path.join(CSRC, "..", "_lib", "asan", "field_loss_rows_asan")


@pytest.fixture(scope="module")
def exe():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asan-field-loss"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.exists(EXE)
    return EXE


@pytest.mark.parametrize("n", [4, 97, 19353])
def test_field_loss_rows_under_asan_ubsan(exe, n):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, str(n)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    got = {line.split()[0]: line.split()[1:] for line in r.stdout.strip().splitlines()}
    n_desc = (n + 1) // 2
    valid = (("all", n), ("null_rows", n), ("null_rows_weights", n), ("one", 1), ("descending", n_desc),
             ("prefix", 33 if n > 33 else n // 2), ("one_weight_left", n), ("cotangent", n_desc))
    for name, count in valid:
        assert got[name][0] == "ok" and int(got[name][1]) == count, (name, got[name])
    refused = {"repeat_adjacent": "repeats", "repeat_ends": "repeats", "repeat_after_all": "repeats",
               "index_n": "outside", "index_minus_one": "outside", "index_int_min": "outside",
               "index_int_max": "outside", "empty_perm_row": "outside", "no_rows": "least", "negative_count": "least",
               "empty_perm": "no", "weights_zero": "zero", "weights_zero_selected": "zero",
               "weight_negative": "negative", "weight_nan": "negative", "weight_inf": "negative",
               "weights_cotangent": "PFR_LOSS_FCOTANGENT"}
    for name, word in refused.items():
        assert got[name][0] == "refused" and word in got[name], (name, got[name])
    assert len(got) == len(valid) + len(refused)
