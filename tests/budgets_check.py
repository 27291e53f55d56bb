"""Shared by tests/test_budgets_host.py and tests/test_budgets_trace_gpu.py: the recorder of budget traces
(tests/golden/make_budgets_trace.py) as a module, and the build of tests/budgets_host_check.cpp with the host compiler."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def trace_tool():
    spec = importlib.util.spec_from_file_location("make_budgets_trace", os.path.join(GOLDEN, "make_budgets_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_check(exe, sanitize):
    """sanitize: AddressSanitizer + UBSan, exactly as tests/test_setup_host.py builds its program"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++ or clang++)")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
        if "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
            cmd[1:1] = ["-static-libasan", "-static-libubsan"]     # gcc: the runtimes inside the program, as clang links them
    cmd += ["-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "budgets_host_check.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe
