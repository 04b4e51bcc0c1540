"""The CPU emulation of every kernel family under AddressSanitizer and UBSan ("Sanitized emulation run").

tests/emu_sanitized_check.cpp is an ordinary executable with its own main that calls the C-ABI only.  `make -C tests/hipemu asan`
compiles the six product sources against the emulation header with -fsanitize=address,undefined -fno-sanitize-recover=all, as
separate objects (seven translation units with the driver: one make job each), and links the driver.  hipMalloc is a malloc of
exactly the requested size there and a workgroup's dynamic LDS a heap block of exactly the launch's byte count, so an index that
runs off a device buffer is a report, not a plausible number.  The driver runs each scenario in a context of its own at the
sizes where an index can run off the end, checks return codes, finiteness, the symmetry of Sigma and the slot statistics, and
fails unless every profile span ran.  Nothing is preloaded and no sanitizer option is set: every check, leak detection included,
stays on.
A host-only check: it runs where there is no GPU.

Measured where this was written (8 cores): the build 5 min 36 s to 6 min 34 s in parallel (ekf_window.hip alone is 5 min 42 s),
8 min 53 s serial; the driver 32.7 s and 37.2 s in two runs on the idle machine.  DRIVER_SECONDS is the larger figure and the
driver's time limit three times that: the margin is for a loaded machine."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SECONDS = 37
JOBS = 7                                                    # six product sources and the driver


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="host-only sanitizer check: runs on machines without a GPU")
def test_emu_sanitized_check():
    emu = os.path.join(ROOT, "tests", "hipemu")
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS", "LSAN_OPTIONS")}   # no check switched off
    b = subprocess.run(["make", "-C", emu, f"-j{JOBS}", "asan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert b.returncode == 0, b.stdout[-4000:]
    r = subprocess.run([os.path.join(emu, "_build", "asan", "emu_sanitized_check")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, env=env, timeout=3 * DRIVER_SECONDS)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("emu_sanitized_check ok"), r.stdout[-4000:]
