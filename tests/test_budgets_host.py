"""The launch-budget policy and the verdict after a map (nekstab_amd/csrc/nsk_budgets_host.hpp), checked by a stand-alone program
(tests/budgets_host_check.cpp) built with the host compiler under AddressSanitizer and UBSan: the properties the module's
comments promise, the verdict table, and the replay of tests/golden/budgets_trace.txt -- what the library did on an MI355X at the
commit before the module existed (tests/golden/make_budgets_trace.py), reproduced to the integer."""
import json
import os
import subprocess

from tests.budgets_check import GOLDEN, build_check, trace_tool


def test_text_twin_is_the_recorded_trace():
    """budgets_trace.txt (what the C++ program reads) holds exactly what budgets_trace.json holds, and the recording is the one the
    issue asks for: 12 direct maps of 20 steps and 4 adjoint maps in one context, a second direct chain with tail = 0."""
    with open(os.path.join(GOLDEN, "budgets_trace.json")) as fh:
        trace = json.load(fh)
    with open(os.path.join(GOLDEN, "budgets_trace.txt")) as fh:
        assert fh.read() == trace_tool().text_twin(trace)
    a, b = trace["contexts"]
    assert [m["kind"] for m in a["maps"]] == [0] * 12 + [1] * 4 and a["tail"] == -1 and a["net"] == 1 and a["nsteps"] == 20
    assert [m["kind"] for m in b["maps"]] == [0] * 10 and b["tail"] == 0 and b["net"] == 0
    assert all(len(m["iters_h"]) == 20 and min(m["attempts"][-1]["helm_max"]) > 0 for c in (a, b) for m in c["maps"])      # all six classes ran
    assert a["maps"][-1]["sb_maps"] >= 12 and b["maps"][-1]["sb_maps"] >= 8                                              # per-step budgets in use


def test_budgets_module_under_sanitizers(tmp_path):
    exe = build_check(str(tmp_path / "budgets_host_check"), sanitize=True)
    r = subprocess.run([exe, os.path.join(GOLDEN, "budgets_trace.txt")], capture_output=True, text=True)      # a stand-alone program: nothing is preloaded for it
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert "budgets_host_check ok" in r.stdout
