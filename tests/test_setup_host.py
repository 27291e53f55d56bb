"""The host set-up steps shared by build, build3 and shard_fill (nekstab_amd/csrc/nsk_setup_host.hpp): the gather-scatter CSR, the
four-integer table rows, dssum_h, corner_table and sort_gid_pairs, checked by a stand-alone program (tests/setup_host_check.cpp)
built with the host compiler under AddressSanitizer and UBSan.  A wrong entry of these tables is an out-of-bounds load on the
device."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_setup_host_tables_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++, c++ or clang++)")
    exe = str(tmp_path / "setup_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "setup_host_check.cpp")]
    if "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout:
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]     # gcc: the runtimes inside the program, as clang links them
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)             # a stand-alone program: nothing is preloaded for it
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert "setup_host_check ok" in r.stdout
