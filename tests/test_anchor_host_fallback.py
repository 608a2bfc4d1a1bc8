"""CPU: the one branch of the anchor stage that no backend reaches on its own -- the device join reports unstable occurrence
groups and the whole stage is redone on the host (host index built then, for the first time; host join after it).  The
harness installs a device anchor path that always declines (DG_HARNESS_UNSTABLE_ANCHORS: 0 minimizers per haplotype, an
empty result with n_unstable_groups = 1); the Anchor_hits dump must be the plain host path's, byte for byte, both must be
the reference's (tests/golden/anchors.json), and the FASTA the reference's (tests/golden/e2e.json).  The "Number of
Minimizers" lines differ by design (the stub's counts are printed before the redo), so stderr is not compared."""
import hashlib
import os
import subprocess

import pytest

from test_anchors_golden import ANCH, CASES, ROOT, check_dump

# a diploid bubble panel, a case off the default (k, w), and one whose shared-anchor filter drops ids (-T0.75)
NAMES = ["bub_a", "kw_k8_w130", "bub_h"]


def run(built_cpu, c, tmp, tag, env):
    dump, fa = tmp / f"{tag}.txt", tmp / f"{tag}.fa"
    p = subprocess.run([built_cpu, "-t4", *c["args"], "-g", os.path.join(ROOT, c["gfa"]), "-r", os.path.join(ROOT, c["reads"]), "-o", str(fa), "-A", str(dump)],
                       check=True, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return dump, open(fa, "rb").read(), p.stderr.decode()


@pytest.mark.parametrize("name", NAMES)
def test_unstable_device_join_is_redone_on_the_host(name, built_cpu, tmp_path):
    c, a = CASES[name], ANCH[name]
    assert [f"-k{a['k']}", f"-w{a['w']}"] == [x for x in c["args"] if x[:2] in ("-k", "-w")]
    env = {k: v for k, v in os.environ.items() if k != "DG_HARNESS_UNSTABLE_ANCHORS"}
    host_dump, host_fa, host_err = run(built_cpu, c, tmp_path, "host", env)
    redo_dump, redo_fa, redo_err = run(built_cpu, c, tmp_path, "redo", dict(env, DG_HARNESS_UNSTABLE_ANCHORS="1"))
    assert "redoing the stage on the host" in redo_err and "redoing the stage on the host" not in host_err
    assert open(redo_dump, "rb").read() == open(host_dump, "rb").read()
    check_dump(host_dump, a)
    check_dump(redo_dump, a)
    assert hashlib.md5(host_fa).hexdigest() == c["fasta_md5"] and redo_fa == host_fa
