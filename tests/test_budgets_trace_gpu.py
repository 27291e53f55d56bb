"""The launch budgets the library RUNS with are what nekstab_amd/csrc/nsk_budgets_host.hpp predicts from the library's own
iteration counts: the first chain of tests/golden/make_budgets_trace.py (12 direct maps of 20 steps on the cylinder fixture at
lx1 = 6, a production context, in a child process with NSK_DEBUG=2) handed to the replay of tests/budgets_host_check.cpp.  This is
the wiring -- nsk.hip feeding the module the counters of the map it just ran, and launching what the module answers -- whatever
iteration counts a future kernel produces."""
import subprocess

import pytest

from tests.budgets_check import build_check, trace_tool

pytestmark = pytest.mark.gpu


def test_library_runs_the_budgets_the_module_predicts(tmp_path):
    tool = trace_tool()
    trace, _ = tool.record("first", timeout=120)               # a fresh child under a time limit
    (ctx,) = trace["contexts"]
    maps = ctx["maps"]
    assert len(maps) == 12 and all(m["kind"] == 0 and len(m["iters_h"]) == 20 for m in maps)
    assert all(len(m["attempts"]) >= 1 for m in maps), "no `map:` line for a map: NSK_DEBUG=2 did not reach the library"
    assert maps[-1]["retries"] == 0 and all(len(m["attempts"]) == 1 and m["attempts"][0]["unconverged"] == 0 for m in maps)
    assert all(m["finite"] for m in maps)
    assert maps[-1]["sb_maps"] == 11 and ctx["net"] == 1        # per-step budgets behind the safety-net tail from the second map on
    txt = tmp_path / "trace.txt"
    txt.write_text(tool.text_twin(trace))
    exe = build_check(str(tmp_path / "budgets_host_check"), sanitize=False)
    r = subprocess.run([exe, "--replay", str(txt)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr
    assert "budgets_host_check ok" in r.stdout
