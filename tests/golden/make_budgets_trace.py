"""Records tests/golden/budgets_trace.json (+ its flat text twin budgets_trace.txt, which tests/budgets_host_check.cpp
reads): what the launch-budget policy of the library did over chains of maps on the cylinder fixture at lx1 = 6.

    python tests/golden/make_budgets_trace.py [--out DIR] [--chains first|all] [--sharded]

The maps run in a FRESH CHILD process with NSK_DEBUG=2 (every other NSK_* variable but NSK_LIB removed); the child writes one
`@@map {json}` line to stderr behind every map, so the library's own `map:` lines (one per attempt: unconverged solves, per
step class the largest iteration count / the class budget the attempt held) and the records interleave in order.

Per context: the caps and options the budgets depend on; per map: kind (0 direct, 1 adjoint), the attempts of the `map:`
lines, step_iters(), retries, recaptures, budget_helm / budget_pres, and the cumulative budgeted launches of the per-step
budgets, round(step_budget_*_mean x step_budget_maps x nsteps).  The SHA-256 of the last downloaded vector closes a context.

Chains (`all`): context A = 12 direct maps of 20 steps (all six step classes, the 8-map window fills, per-step budgets behind
the safety-net tail) followed by 4 adjoint maps; context B = option tail = 0, 10 direct maps (the head-room of plain budgets).
`first` is context A's direct chain alone (tests/test_budgets_trace_gpu.py).  --sharded: two virtual ranks, 10 maps, step graphs
and shard_graph = 0 (budget_helm / budget_pres / retries / recaptures / hash only: shards keep no per-step record).
"""
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NSTEPS = 20
CLS_FIELDS = ("helm_max", "helm_budget", "pres_max", "pres_budget")


def _sha(parts):
    import numpy as np
    h = hashlib.sha256()
    for a in parts:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()


def _note(rec):
    sys.stderr.write("@@map " + json.dumps(rec) + "\n")
    sys.stderr.flush()


def _chain(h, kinds, nsteps):
    """q <- map(q) / |map(q)|, len(kinds) times; one record per map; returns the last vector's hash"""
    import numpy as np
    from nekstab_amd import seed
    qx, qy = seed.add_noise(h.case)
    q, f = h.alloc(2)
    h.upload(q, qx, qy, np.zeros(h.npres))
    h.scal(q, 1.0 / h.norm(q))
    h.set_nsteps(nsteps)
    for kind in kinds:
        h.matvec(f, q, kind)
        st = h.stats()
        hh, pp = h.step_iters()
        nrm = h.norm(f)
        _note({"kind": kind, "iters_h": [int(x) for x in hh], "iters_p": [int(x) for x in pp], "retries": st["retries"],
               "recaptures": st["recaptures"], "budget_helm": st["budget_helm"], "budget_pres": st["budget_pres"],
               "sb_maps": st["step_budget_maps"], "tail_maps": st["tail_maps"], "finite": bool(np.isfinite(nrm)),
               "sb_launch_h": int(round(st["step_budget_helm_mean"] * st["step_budget_maps"] * nsteps)),
               "sb_launch_p": int(round(st["step_budget_pres_mean"] * st["step_budget_maps"] * nsteps))})
        h.scal(f, 1.0 / nrm)
        q, f = f, q
    return _sha(h.download(q))


def _child(which):
    import numpy as np                                          # noqa: F401
    from nekstab_amd import mesh
    from nekstab_amd.settings import PRODUCTION, PRODUCTION_OPTIONS, production_context
    case = mesh.load_case_npz(os.path.join(ROOT, "tests", "golden", "cylinder_case.npz"), 6)
    base = {"max_helm": PRODUCTION["max_helm_iter"], "max_pres": PRODUCTION["max_pres_iter"], "min_pres": PRODUCTION_OPTIONS["min_pres_iter"],
            "nsteps": NSTEPS, "tail_off_h": 0, "tail_off_p": 0, "sb_pct": 90, "bhead": 3, "sb_head_h": -1, "sb_head_p": -1}
    if which == "sharded":
        from nekstab_amd.sharded import ShardGroup
        for sg in (-1, 0):
            h = production_context(case)
            g = ShardGroup(h, case, 2)
            g.set_option("shard_graph", sg)
            g.set_nsteps(NSTEPS)
            sys.stderr.write("@@context " + json.dumps(dict(base, tail=-1, shard_graph=sg, ranks=2)) + "\n"); sys.stderr.flush()
            from nekstab_amd import seed
            qx, qy = seed.add_noise(case)
            q, f = g.alloc(2)
            g.upload(q, qx, qy, np.zeros((case.nel, 4, 4)))
            g.scal(q, 1.0 / g.norm(q))
            for _ in range(10):
                g.matvec(f, q, 0)
                st = g.stats()
                st = st[0] if isinstance(st, (list, tuple)) else st
                nrm = g.norm(f)
                _note({"kind": 0, "retries": st["retries"], "recaptures": st["recaptures"], "budget_helm": st["budget_helm"],
                       "budget_pres": st["budget_pres"], "finite": bool(np.isfinite(nrm))})
                g.scal(f, 1.0 / nrm)
                q, f = f, q
            sys.stderr.write("@@end " + json.dumps({"vector_sha256": _sha(g.download(q))}) + "\n"); sys.stderr.flush()
            g.close(); h.close()
        return
    for tail, kinds in ((-1, [0] * 12 + ([1] * 4 if which == "all" else [])),) + (((0, [0] * 10),) if which == "all" else ()):
        h = production_context(case)
        h.case = case
        if tail != -1:
            h.set_option("tail", tail)
        sys.stderr.write("@@context " + json.dumps(dict(base, tail=tail)) + "\n"); sys.stderr.flush()
        sha = _chain(h, kinds, NSTEPS)
        sys.stderr.write("@@end " + json.dumps({"vector_sha256": sha}) + "\n"); sys.stderr.flush()
        h.close()


_MAP = re.compile(r"^map: unconverged (\d+) \| helm max/budget((?: \d+/\d+)+) \| pres max/budget((?: \d+/\d+)+)\s*$")


def parse(stderr_text):
    """the child's stderr -> {"contexts": [...]}"""
    ctxs, attempts = [], []
    for line in stderr_text.splitlines():
        m = _MAP.match(line)
        if m:
            hp = [[int(x) for x in t.split("/")] for t in m.group(2).split()]
            pp = [[int(x) for x in t.split("/")] for t in m.group(3).split()]
            attempts.append({"unconverged": int(m.group(1)), "helm_max": [a for a, _ in hp], "helm_budget": [b for _, b in hp],
                             "pres_max": [a for a, _ in pp], "pres_budget": [b for _, b in pp]})
        elif line.startswith("@@context "):
            ctxs.append(dict(json.loads(line[10:]), maps=[]))
            attempts = []
        elif line.startswith("@@map "):
            ctxs[-1]["maps"].append(dict(json.loads(line[6:]), attempts=attempts))
            attempts = []
        elif line.startswith("@@end "):
            ctxs[-1].update(json.loads(line[6:]))
    for c in ctxs:                                              # the safety-net tail runs or not for a whole context
        c["net"] = int(any(m.get("tail_maps", 0) > 0 for m in c["maps"]))
    return {"contexts": ctxs}


def record(which="all", timeout=240):
    """run the chains in a fresh child; returns (trace, the child's stderr)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("NSK_") or k == "NSK_LIB"}      # (NSK_LIB: which build to record)
    if which != "sharded":                                      # (shards print no `map:` line; their debug output is per step and rank)
        env["NSK_DEBUG"] = "2"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which], env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("trace child failed (%d):\n%s" % (r.returncode, r.stderr[-4000:]))
    return parse(r.stderr), r.stderr


def text_twin(trace):
    """the flat form tests/budgets_host_check.cpp reads: whitespace-separated integers behind a keyword per line"""
    out = []
    for c in trace["contexts"]:
        if "ranks" in c:
            continue
        out.append("context %d %d %d %d %d %d %d %d %d %d %d %d %d" % (c["max_helm"], c["max_pres"], c["min_pres"], c["nsteps"], c["tail"], c["net"],
                   c["tail_off_h"], c["tail_off_p"], c["sb_pct"], c["bhead"], c["sb_head_h"], c["sb_head_p"], len(c["maps"])))
        for m in c["maps"]:
            out.append("map %d %d %d %d %d %d %d" % (m["kind"], len(m["attempts"]), m["sb_maps"], m["sb_launch_h"], m["sb_launch_p"], m["retries"], len(m["iters_h"])))
            for a in m["attempts"]:
                out.append("attempt %d " % a["unconverged"] + " ".join(" ".join(str(x) for x in a[k]) for k in CLS_FIELDS))
            out.append("iters_h " + " ".join(str(x) for x in m["iters_h"]))
            out.append("iters_p " + " ".join(str(x) for x in m["iters_p"]))
    return "\n".join(out) + "\n"


def main(argv):
    if len(argv) >= 2 and argv[0] == "--child":
        _child(argv[1])
        return 0
    out = os.path.dirname(os.path.abspath(__file__))
    which = "all"
    for i, a in enumerate(argv):
        if a == "--out":
            out = argv[i + 1]
        if a == "--chains":
            which = argv[i + 1]
        if a == "--sharded":
            which = "sharded"
    trace, _ = record(which)
    os.makedirs(out, exist_ok=True)
    stem = "budgets_trace" + ("_sharded" if which == "sharded" else "")
    with open(os.path.join(out, stem + ".json"), "w") as fh:
        json.dump(trace, fh, indent=None, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    if which != "sharded":
        with open(os.path.join(out, "budgets_trace.txt"), "w") as fh:
            fh.write(text_twin(trace))
    for c in trace["contexts"]:
        print("context tail", c["tail"], "maps", len(c["maps"]), "retries", c["maps"][-1]["retries"], "recaptures", c["maps"][-1]["recaptures"],
              "budgets", c["maps"][-1]["budget_helm"], c["maps"][-1]["budget_pres"], "sha256", c.get("vector_sha256"))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
