#!/usr/bin/env python3
"""A timed read-tagging pass on the bench's synthetic MHC-24 read set against the two walks the reads were drawn from, beside the
scoring pass (dg_sketch_reads) on the same reads in the same process, the two alternating: python tools/tag_perf.py [reps]
Prints the last (warm) pass of each and the median and range over the warm passes."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from dipgenie_amd import capi, synth
K, W, SAMPLE = 31, 25, (5, 6)                                          # synth.mosaic_panel draws the reads from walks 5 and 6
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
gfa, reads_path, info = synth.ensure_mhc24("/tmp/mhc24")
reads = [r for r in open(reads_path, "rb").read().split(b"\n")[1::2] if r]
names, seqs, links, walks = synth.parse_gfa(gfa)
haps = [b"".join(seqs[v] for v in walks[h][2]).upper() for h in SAMPLE]
off = np.zeros(len(reads) + 1, np.int64); np.cumsum([len(r) for r in reads], out=off[1:])
bases = b"".join(reads)
ctx = capi.Context(0)
ha, hb = (ctx.sketch_haplotype(h, K, W)[0] for h in haps)


def timing():
    t = ctx.sketch_timing()
    return (t.kernel_ms, t.sort_ms, t.total_ms, t.n_emitted)


score, tag, dedup, dic = [], [], [], []
for it in range(REPS + 1):                                             # the first pass is the cold one: not counted
    ctx.sketch_reads_flat(bases, off, K, W); score.append(timing())
    rec = ctx.sketch_tag_reads_flat(bases, off, K, W, ha, hb); tag.append(timing())
    # where sort_ms goes: empty lists leave the per-read dedup (every probe ends at once), one read leaves the dictionary; the rest is the probes
    ctx.sketch_tag_reads_flat(bases, off, K, W, ha[:0], hb[:0]); dedup.append(timing()[1])
    ctx.sketch_tag_reads_flat(bases[:off[1]], off[:2], K, W, ha, hb); dic.append(timing()[1])
rec = ctx.sketch_tag_reads_flat(bases, off, K, W, ha, hb)
stat = {s: ctx.sketch_stat(s) for s in ("tag_long_reads", "tag_dict_distinct", "tag_table_slots")}
med = lambda xs: f"{np.median(xs[1:]):.3f} ({min(xs[1:]):.3f}-{max(xs[1:]):.3f})"
col = lambda rows, i: [r[i] for r in rows]
which = np.where(rec[:, 1] > rec[:, 2], 1, np.where(rec[:, 2] > rec[:, 1], 2, 0))
print(f"{len(reads)} reads ({off[-1] / 1e6:.1f} Mbp), k {K} w {W}; lists {ha.size} + {hb.size} hashes, {stat}")
print(f"tag pass, last:     kernel_ms {tag[-1][0]:.3f} (tile pass) sort_ms {tag[-1][1]:.3f} (dictionary + tagging) total_ms {tag[-1][2]:.3f}; emitted {tag[-1][3]}")
print(f"scoring pass, last: kernel_ms {score[-1][0]:.3f} sort_ms {score[-1][1]:.3f} total_ms {score[-1][2]:.3f}; emitted {score[-1][3]}   (dg_sketch_reads, same reads, same process)")
print(f"median (range) of {REPS} warm passes, ms:")
print(f"  tag pass:     kernel_ms {med(col(tag, 0))} sort_ms {med(col(tag, 1))} total_ms {med(col(tag, 2))}")
print(f"  scoring pass: kernel_ms {med(col(score, 0))} sort_ms {med(col(score, 1))} total_ms {med(col(score, 2))}")
print(f"  of the tag pass's sort_ms: dictionary {med(dic)} (a one-read call with the same lists), dedup {med(dedup)} (empty lists), "
      f"probes ~{np.median(col(tag, 1)[1:]) - np.median(dic[1:]) - np.median(dedup[1:]):.3f} (the rest)")
print(f"tag / scoring total (medians): {np.median(col(tag, 2)[1:]) / np.median(col(score, 2)[1:]):.2f}x; reads tagged 1: {(which == 1).sum()}, 2: {(which == 2).sum()}, "
      f"tie: {((which == 0) & (rec[:, 1] > 0)).sum()}, no evidence: {((rec[:, 1] == 0) & (rec[:, 2] == 0)).sum()}")
