"""Sanitizer run of pruning's host code (tests/test_asan_host.py builds and describes the driver): the stand-alone
``symbolic_asan --forest`` builds a forest of three elimination trees under AddressSanitizer + UndefinedBehaviorSanitizer,
puts a load in the first tree and sensor rows in the first two, and has the plan and schedule of the loaded view and of
its complement checked for every engine shape (``pfr::check_plan``, ``pfr::check_schedule``).  The plate patterns'
views are checked by the driver's ordinary runs (tests/test_asan_host.py)."""
import os
import subprocess

from test_asan_host import CSRC, EXE


def test_forest_views_under_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asan-host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([EXE, "--forest"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.stdout.strip() == "forest ok 81", r.stdout[-2000:]
