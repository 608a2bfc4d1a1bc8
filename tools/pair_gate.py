#!/usr/bin/env python3
"""In-situ measurement of the level-pair options: for every setting (k=v,k=v;...) load the graph anew -- the pair options take effect at
the load -- and run n passes (default 4; the first of a setting captures its hipGraph batches), printing the forward sweep by HIP
events, the launch count and the pair profile:  python tools/pair_gate.py graph.dpg "pair_wide=0;pair_wide=1,pair_wide_rc=4" [n]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import capi
ctx = capi.Context(0)
g = capi.DpGraphArrays.load(sys.argv[1])
settings = [dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in st.split(",") if kv) for st in sys.argv[2].split(";")]
n = int(sys.argv[3]) if len(sys.argv) > 3 else 4
ref = None
for st in settings:
    with ctx.dp_options(**st):
        t0 = time.time()
        ctx.dp_load_graph(g)
        load_s = time.time() - t0
        fwd = []
        for _ in range(n):
            out = ctx.dp_run()
            tm = ctx.dp_timing()
            fwd.append(round(tm.forward_ms, 2))
            ref = ref or out.key()
            assert out.key() == ref, st
        pairs = ctx.dp_pair_profile()
        print(" ".join(f"{k} {v}" for k, v in st.items()) or "defaults", f": load {load_s:.3f} s  fwd_ms min {min(fwd)} all {fwd}  launches {int(tm.n_forward_launches)}  pairs {sum(pairs.values())}"
              f" (wide {sum(v for k, v in pairs.items() if 'wide' in k)})  value {out.value}  {json.dumps(pairs)}", flush=True)
