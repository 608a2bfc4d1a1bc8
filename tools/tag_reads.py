#!/usr/bin/env python3
"""Tag a read set against any two sequences: python tools/tag_reads.py HAPS.fa READS.fq -k K -w W > tags.tsv

HAPS.fa holds the two sequences (its first two records); READS is FASTA or FASTQ, plain or gzip.  One row per read in input order:
read, length, n_min, only_1, only_2, both, tag -- the table bin/DipGenie --tag-reads writes, from dg_sketch_tag_reads through capi."""
import argparse, gzip, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dipgenie_amd import capi


def records(path):
    """(name, sequence) per FASTA / FASTQ record; the name ends at the first white space"""
    with (gzip.open if path.endswith(".gz") else open)(path, "rb") as f:
        lines = [ln.rstrip(b"\r\n") for ln in f]
    i, out = 0, []
    while i < len(lines):
        ln = lines[i]
        if not ln or ln[:1] not in (b">", b"@"):
            i += 1
            continue
        fastq, name, seq = ln[:1] == b"@", (ln[1:].split() or [b""])[0].decode(), []
        i += 1
        while i < len(lines) and lines[i][:1] not in ((b"+",) if fastq else (b">", b"@")):
            seq.append(lines[i]); i += 1
        seq = b"".join(seq)
        if fastq:                                                      # the '+' line, then as many quality bytes as bases
            i += 1
            q = 0
            while i < len(lines) and q < len(seq):
                q += len(lines[i]); i += 1
        out.append((name, seq))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("haps"); ap.add_argument("reads")
    ap.add_argument("-k", type=int, default=31); ap.add_argument("-w", type=int, default=25); ap.add_argument("-G", type=int, default=0, help="device")
    a = ap.parse_args()
    haps = records(a.haps)
    if len(haps) < 2:
        sys.exit(f"{a.haps}: two sequences needed, {len(haps)} found")
    reads = records(a.reads)
    ctx = capi.Context(a.G)
    ha, hb = (ctx.sketch_haplotype(s, a.k, a.w)[0] for _, s in haps[:2])
    rec = ctx.sketch_tag_reads([s for _, s in reads], a.k, a.w, ha, hb)
    out = ["read\tlength\tn_min\tonly_1\tonly_2\tboth\ttag"]
    for (name, s), (n_min, o1, o2, both) in zip(reads, rec.tolist()):
        out.append(f"{name}\t{len(s)}\t{n_min}\t{o1}\t{o2}\t{both}\t{1 if o1 > o2 else 2 if o2 > o1 else 0}")
    sys.stdout.write("\n".join(out) + "\n")
    t = ctx.sketch_timing()
    print(f"{len(reads)} reads against {haps[0][0]} ({ha.size} minimizers) and {haps[1][0]} ({hb.size}): tile pass {t.kernel_ms:.3f} ms, dictionary + tagging {t.sort_ms:.3f} ms",
          file=sys.stderr)


if __name__ == "__main__":
    main()
