"""CPU tests of the test option "alloc_fill" (include/eppm_test.h): its argument check, and that the switch lives in the two test libraries
alone -- the product and the tolerance library export no test symbol and are linked from the objects they were linked from before, with
mem_cache_test.o the one object the option adds to a test library.  What the option is for: tests/test_alloc_fill_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import eppm_amd
from conftest import ROOT
from eppm_amd import _lib

ARG = 1


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_alloc_fill_takes_off_or_a_byte():
    L = eppm_amd.lib()
    assert L._name == eppm_amd.lib_path("test")
    try:
        for v in (-1, 0, 255):
            assert L.eppm_test_set_option(b"alloc_fill", v) == 0, v
        for v in (-2, 256, 1 << 20, -(1 << 31)):
            assert L.eppm_test_set_option(b"alloc_fill", v) == ARG, v
            assert b"alloc_fill" in L.eppm_last_error()
    finally:
        assert L.eppm_test_set_option(b"alloc_fill", -1) == 0
    T = C.CDLL(eppm_amd.lib_path("tol_test"))
    assert T.eppm_test_set_option(b"alloc_fill", 255) == 0 and T.eppm_test_set_option(b"alloc_fill", 256) == ARG
    assert T.eppm_test_set_option(b"alloc_fill", -1) == 0


def test_the_fill_lives_in_the_test_libraries_only():
    for variant in ("", "tol"):
        syms = _exported(eppm_amd.lib_path(variant))
        assert not (syms & set(_lib.TEST_SYMBOLS)), variant
        assert not [s for s in syms if s.startswith("eppm_test") or s.startswith("eppm_probe") or "alloc_fill" in s], variant
    for variant in ("test", "tol_test"):
        assert not [s for s in _exported(eppm_amd.lib_path(variant)) if "alloc_fill" in s], variant        # hidden there too: a helper, no ABI
    mk = open(os.path.join(ROOT, "eppm_amd", "csrc", "Makefile")).read()
    hooked = " ".join(re.findall(r"^HOOKED \+?= ([^#\n]*)", mk, flags=re.M)).split()
    assert sorted(hooked) == ["context", "launchers_ref_abi", "mem_cache", "rng_tables"], hooked
    # the product build has no fill: the option is a constant there, and the helper is declared under EPPM_TEST_HOOKS alone
    hdr = open(os.path.join(ROOT, "eppm_amd", "csrc", "api_internal.h")).read()
    hooks, product = hdr.split("#ifdef EPPM_TEST_HOOKS")[1].split("#else")[0], hdr.split("#ifdef EPPM_TEST_HOOKS")[1].split("#else")[1].split("#endif")[0]
    assert "alloc_fill(hipError_t" in hooks and "alloc_fill(hipError_t" not in product
    assert "static constexpr int opt_alloc_fill() { return -1; }" in product
    csrc = os.path.join(ROOT, "eppm_amd", "csrc")
    callers = {f[:-4] for f in os.listdir(csrc) if f.endswith(".cpp") and f != "test_hooks.cpp" and re.search(r"\balloc_fill\(", open(os.path.join(csrc, f)).read())}
    assert callers == {"rng_tables", "mem_cache", "launchers_ref_abi"}, callers
