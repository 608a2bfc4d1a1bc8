#!/usr/bin/env python3
"""Two builds of the product CLI on the MHC-24 bench input, alternating, on one GPU: per [dg::stage] line and for `total`
(wall of the process) the median of each build and the first build's min-max spread; the second build passes a stage when
its median lies inside that spread.  The FASTA of every run must be the same.
usage: python tools/cli_ab.py <parent DipGenie> <child DipGenie> [reps=5] [gap seconds=3]"""
import hashlib, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import synth
bins = {"parent": sys.argv[1], "child": sys.argv[2]}
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
gap = float(sys.argv[4]) if len(sys.argv) > 4 else 3.0
d = "/tmp/dg_bench_cache/mhc24"
gfa, reads, info = synth.ensure_mhc24(d)
times = {k: {} for k in bins}
md5 = set()
for rep in range(reps + 1):                                     # (round 0 warms the file cache and is not counted)
    for who, exe in bins.items():
        t0 = time.time()
        p = subprocess.run([exe, "-t16", "-p2", "-R18", "-g", gfa, "-r", reads, "-o", f"{d}/ab.fa"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
        wall = time.time() - t0
        if p.returncode != 0: sys.exit(f"{who} run {rep}: exit {p.returncode}\n{p.stderr.decode()[-2000:]}")
        md5.add(hashlib.md5(open(f"{d}/ab.fa", "rb").read()).hexdigest())
        if rep:
            times[who].setdefault("total", []).append(wall)
            for name, s in re.findall(r"\[dg::stage\] (.*?)\s+([0-9.]+) s", p.stderr.decode()): times[who].setdefault(name, []).append(float(s))
        print(f"round {rep} {who}: wall {wall:.3f} s", flush=True)
        time.sleep(gap)
print(f"FASTA md5 over all runs: {sorted(md5)}")
print(f"{'stage':30s} {'parent med':>10s} {'parent min':>10s} {'parent max':>10s} {'child med':>10s}  verdict")
ok = len(md5) == 1
for name, a in times["parent"].items():
    b = times["child"].get(name, [float("nan")])
    inside = min(a) <= statistics.median(b) <= max(a)
    faster = statistics.median(b) < min(a)
    ok = ok and (inside or faster)
    print(f"{name:30s} {statistics.median(a):10.3f} {min(a):10.3f} {max(a):10.3f} {statistics.median(b):10.3f}  {'inside' if inside else 'below' if faster else 'ABOVE'}")
sys.exit(0 if ok else 1)
