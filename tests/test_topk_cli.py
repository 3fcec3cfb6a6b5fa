"""./pagerank --topk K: after the last batch, one line per entry of every source (topk <source> <rank> <vertex> <p>),
in source order, through the device-side selection; the order derived from --dump agrees. Without the flag stdout has
no such line."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen
from tests.test_cli import pagerank, read_dump, run, small_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

K = 20


def topk_lines(stdout):
    return [l for l in stdout.splitlines() if l.startswith("topk ")]


def check_against_dumps(stdout, dumps, sources):
    lines = topk_lines(stdout)
    got = [tuple(l.split()[1:]) for l in lines]
    order = [sources.index(int(g[0])) for g in got]
    assert order == sorted(order)  # in source order
    for s in sources:
        p = dumps[s][0]
        ids = np.nonzero(p > 0)[0]
        want = ids[np.lexsort((ids, -p[ids]))][:K]
        mine = [g for g in got if int(g[0]) == s]
        assert [int(g[1]) for g in mine] == list(range(1, len(want) + 1))
        assert [int(g[2]) for g in mine] == [int(v) for v in want]
        assert all(float(g[3]) == p[v] for g, v in zip(mine, want))  # (%.17g round-trips a double)


def base_args(path):
    return ["-d", path, "-a", "0", "-i", "0", "-y", "1", "-n", "0", "-r", "0.01", "-b", "4"]


def test_one_source(pagerank, small_bin, tmp_path):
    path, V, e1, e2 = small_bin
    src = int(datagen.top_sources(V, e1, e2, 600, 0, 1)[0])
    dump = str(tmp_path / "out.dump")
    r = run([pagerank] + base_args(path) + ["-s", str(src), "--dump", dump, "--topk", str(K)])
    assert r.returncode == 0, r.stdout
    lines = r.stdout.splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith("topk "))
    assert any(l.startswith("id_space ") for l in lines[:first])  # after the report and the id_space line
    assert len(topk_lines(r.stdout)) == K
    check_against_dumps(r.stdout, read_dump(dump), [src])
    plain = run([pagerank] + base_args(path) + ["-s", str(src)])
    assert plain.returncode == 0 and not re.search(r"^topk ", plain.stdout, re.M)


@pytest.mark.parametrize("extra", [[], ["-g", "2", "--share-device"]])
def test_sources_file(pagerank, small_bin, tmp_path, extra):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, 600, 0, 5)]
    sf = tmp_path / "sources.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    dump = str(tmp_path / "out.dump")
    r = run([pagerank] + base_args(path) + ["--sources", str(sf), "--dump", dump, "--topk", str(K)] + extra)
    assert r.returncode == 0, r.stdout
    if extra:
        dumps = {}
        for d in range(2):
            dumps.update(read_dump(f"{dump}.{d}"))
    else:
        dumps = read_dump(dump)
    assert len(topk_lines(r.stdout)) == K * len(sources)
    check_against_dumps(r.stdout, dumps, sources)
    plain = run([pagerank] + base_args(path) + ["--sources", str(sf)] + extra)
    assert plain.returncode == 0 and "topk" not in plain.stdout


def test_out_of_range_k_is_rejected(pagerank, small_bin):
    r = run([pagerank] + base_args(small_bin[0]) + ["--topk", "8193"])
    assert r.returncode != 0 and "invalid arguments" in r.stdout
