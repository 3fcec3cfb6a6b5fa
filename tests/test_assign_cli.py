"""./pagerank --assign on a toy .bin: 20 lines of --target-sets are dealt into two groups (16 + 4 lanes) of one engine; the last
`assign` line and the labels of --assign-out equal the numpy restatement (tests/assign_ref.py) over the vectors --dump writes; the
counts sum to V; every line's flips are those against the line before; without the flag there are no assign lines."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import assign_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"^assign (\d+) classes=(\d+) unassigned=(\d+) flips=(\d+) counts=([\d,]+)$", re.M)


def dump_columns(path):
    """The p vectors of --dump in lane order: [V][lanes]."""
    raw = open(path, "rb").read()
    off, cols = 0, []
    while off < len(raw):
        s, V = np.frombuffer(raw, dtype="<i4", count=2, offset=off)
        off += 8
        cols.append(np.frombuffer(raw, dtype="<f8", count=V, offset=off))
        off += 16 * V
    return np.ascontiguousarray(np.stack(cols, axis=1))


@pytest.mark.parametrize("directed", [1, 0])
def test_cli_assign_over_two_groups_of_target_sets(tmp_path, directed):
    from dynamicppr_amd import datagen
    from tests.test_cli import BIN, run
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "dynamicppr_amd", "host"), "-s", "all"])
    V, e1, e2 = datagen.rmat_stream(9, 6000, 11)
    path = str(tmp_path / "syn.bin")
    datagen.write_bin(path, V, e1, e2)
    rng = np.random.default_rng(8 + directed)
    window = np.unique(np.concatenate([e1[:600], e2[:600]]))
    lines = []
    for lane in range(20):
        ids = rng.choice(window, 1 + lane % 4, replace=False)
        lines.append(" ".join(f"{int(v)}:{0.9 / len(ids):.3f}" if lane % 2 else str(int(v)) for v in ids) if lane % 4 else str(int(ids[0])))
    sf = tmp_path / "sets.txt"
    sf.write_text("\n".join(lines) + "\n")
    dump, labels = str(tmp_path / "out.dump"), str(tmp_path / "labels.bin")
    batches = 4
    base = [BIN, "-d", path, "-a", "0", "-i", str(directed), "-y", "1", "-w", "0.1", "-n", "0", "-r", "0.01", "-b", str(batches),
            "--target-sets", str(sf), "--dump", dump]
    r = run(base + ["--assign", "--assign-out", labels])
    assert r.returncode == 0, r.stdout
    got = LINE.findall(r.stdout)
    assert [int(g[0]) for g in got] == list(range(1, batches + 1)), r.stdout[-2000:]
    P = dump_columns(dump)
    assert P.shape == (V, 20)
    label = ref.assign(P)[0]
    out = np.fromfile(labels, dtype="<i4")
    assert out.shape == (V,) and np.array_equal(out, label)
    want = ref.counts(label, 20)
    b, n_classes, unassigned, flips, counts = got[-1]
    counts = [int(x) for x in counts.split(",")]
    assert int(n_classes) == 20 and counts == want[:20].tolist() and int(unassigned) == int(want[20])
    assert sum(counts) + int(unassigned) == V
    assert np.count_nonzero(label >= 16) > 0          # (the second group's lanes take part)
    # the first line counts against all -1: every assigned vertex is a flip
    first = got[0]
    assert int(first[3]) == V - int(first[2])
    for g in got:
        assert sum(int(x) for x in g[4].split(",")) + int(g[2]) == V
    # a threshold: fewer or as many assigned
    r2 = run(base + ["--assign", "--assign-min", "0.01"])
    assert r2.returncode == 0, r2.stdout
    got2 = LINE.findall(r2.stdout)
    lab2 = ref.assign(P, min_score=0.01)[0]
    assert len(got2) == batches and [int(x) for x in got2[-1][4].split(",")] == ref.counts(lab2, 20)[:20].tolist()
    assert int(got2[-1][2]) == np.count_nonzero(lab2 < 0) >= int(unassigned)
    # without the flag: no assign line
    r3 = run(base)
    assert r3.returncode == 0 and not LINE.findall(r3.stdout) and "assign " not in r3.stdout, r3.stdout[-1000:]
