#!/usr/bin/env python3
"""Two builds of tests/harness/dg_host_oracle (two checkouts of this repository) must behave alike: every fast case of
tests/golden/e2e.json through both, with -A, -D and -J, in four configurations at -t1 and -t4; FASTA, anchor dump, .dpg,
JSON, stdout, exit code and stderr (without the timed [dg::stage] lines) are compared byte for byte.
usage: python tools/host_ab.py <parent checkout> <child checkout>"""
import json, os, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {n: c for n, c in json.load(open(os.path.join(HERE, "tests", "golden", "e2e.json"))).items()
         if not c.get("slow") and not c["gfa"].startswith("<")}
P1 = [n for n, c in CASES.items() if "-p1" in c["args"]]
CONFIGS = [("default", {}, list(CASES)),
           ("graph_literal", {"DG_GRAPH_LITERAL": "1"}, list(CASES)),
           ("levelize_literal", {"DG_LEVELIZE_LITERAL": "1", "DG_GRAPH_LITERAL": "1"}, list(CASES)),
           ("p1", {}, P1)]


def run(root, case, env_extra, threads, work):
    os.makedirs(work)
    cmd = [os.path.join(root, "tests", "harness", "dg_host_oracle"), f"-t{threads}", *case["args"], "-g", os.path.join(HERE, case["gfa"]),
           "-r", os.path.join(HERE, case["reads"]), "-o", "o.fa", "-A", "anchors.txt", "-D", "graph", "-J", "o.json"]
    env = {k: v for k, v in os.environ.items() if k != "DG_DEBUG"}
    p = subprocess.run(cmd, cwd=work, env=dict(env, **env_extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out = {"exit": p.returncode, "stdout": p.stdout,
           "stderr": b"\n".join(l for l in p.stderr.split(b"\n") if not l.startswith(b"[dg::stage]"))}
    for f in ("o.fa", "anchors.txt", "graph.dpg", "o.json"):
        path = os.path.join(work, f)
        out[f] = open(path, "rb").read() if os.path.exists(path) else None
    return out


parent, child = (os.path.abspath(a) for a in sys.argv[1:3])
runs = bad = 0
with tempfile.TemporaryDirectory() as tmp:
    for cfg, env_extra, names in CONFIGS:
        for threads in (1, 4):
            for name in names:
                a = run(parent, CASES[name], env_extra, threads, os.path.join(tmp, f"a_{cfg}_{threads}_{name}"))
                b = run(child, CASES[name], env_extra, threads, os.path.join(tmp, f"b_{cfg}_{threads}_{name}"))
                runs += 1
                diff = [k for k in a if a[k] != b[k]]
                if diff:
                    bad += 1
                    print(f"DIFFERENT {cfg} -t{threads} {name}: {diff}")
            print(f"{cfg} -t{threads}: {len(names)} cases compared", flush=True)
print(f"{runs} parent/child pairs ({len(CASES)} cases, {len(P1)} of them -p1), {bad} different")
sys.exit(1 if bad else 0)
