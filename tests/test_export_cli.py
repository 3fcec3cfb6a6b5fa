"""./pagerank --sparse-min P [--sparse-out FILE]: after the last batch one `support <source> <count>` line per source, in source
order, and in FILE one text line `source id p` per vertex with p > P, by source then id, through the device-side compaction; both
equal numpy over --dump. Without the flag stdout has no such line."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen
from tests.test_cli import pagerank, read_dump, run, small_bin  # noqa: F401  (fixtures)
from tests.test_topk_cli import base_args

pytestmark = pytest.mark.gpu

MIN_P = 1e-6


def check(stdout, text, dumps, sources):
    lines = [l.split() for l in stdout.splitlines() if l.startswith("support ")]
    assert [int(l[1]) for l in lines] == sources  # one line per source, in source order
    rows = [l.split() for l in text.splitlines()]
    at = 0
    for s, line in zip(sources, lines):
        p = dumps[s][0]
        want = np.nonzero(p > MIN_P)[0]
        assert int(line[2]) == len(want) > 0
        mine = rows[at:at + len(want)]
        at += len(want)
        assert [int(r[0]) for r in mine] == [s] * len(want)
        assert [int(r[1]) for r in mine] == [int(v) for v in want]
        assert all(float(r[2]) == p[v] for r, v in zip(mine, want))  # (%.17g round-trips a double)
    assert at == len(rows)


def test_one_source(pagerank, small_bin, tmp_path):
    path, V, e1, e2 = small_bin
    src = int(datagen.top_sources(V, e1, e2, 600, 0, 1)[0])
    dump, out = str(tmp_path / "out.dump"), tmp_path / "sparse.txt"
    r = run([pagerank] + base_args(path) + ["-s", str(src), "--dump", dump, "--sparse-min", str(MIN_P), "--sparse-out", str(out)])
    assert r.returncode == 0, r.stdout
    check(r.stdout, out.read_text(), read_dump(dump), [src])
    plain = run([pagerank] + base_args(path) + ["-s", str(src)])
    assert plain.returncode == 0 and not re.search(r"^support ", plain.stdout, re.M)


@pytest.mark.parametrize("extra", [[], ["-g", "2", "--share-device"]])
def test_sources_file(pagerank, small_bin, tmp_path, extra):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, 600, 0, 5)]
    sf = tmp_path / "sources.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    dump, out = str(tmp_path / "out.dump"), tmp_path / "sparse.txt"
    r = run([pagerank] + base_args(path) + ["--sources", str(sf), "--dump", dump, "--sparse-min", str(MIN_P), "--sparse-out", str(out)] + extra)
    assert r.returncode == 0, r.stdout
    if extra:
        dumps = {}
        for d in range(2):
            dumps.update(read_dump(f"{dump}.{d}"))
    else:
        dumps = read_dump(dump)
    check(r.stdout, out.read_text(), dumps, sources)


def test_bad_arguments_are_rejected(pagerank, small_bin):
    for bad in (["--sparse-min", "-1"], ["--sparse-out", "x.txt"]):
        r = run([pagerank] + base_args(small_bin[0]) + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout
