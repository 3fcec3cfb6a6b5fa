"""./pagerank --subgraph K [--subgraph-out FILE]: after every batch one line `subgraph <source> vertices <L> edges <m>` per source,
through dppr_subgraph / dppr_group_subgraph, and with --subgraph-out the CSR of the last batch as text lines `v <source> <position>
<vertex> <pagerank>` and `e <source> <tail position> <head position>`. The lines of the last batch and the file equal, exactly
(%.17g round-trips a double), the restatement of tests/subgraph_ref.py over the dumped state's order on the same window, and what the
binding's call returns for that state. (Two solves of one stream agree to far below the tolerance, not always to the bit: the earlier
batches are compared by their shape, as in tests/test_cluster_cli.py.) Without the flag stdout has no such line and is otherwise the
same sequence of lines; a bad argument is found before any device work."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from tests import subgraph_ref
from tests.test_changes_cli import BATCHES, SERIAL, W, base_args
from tests.test_cli import pagerank, read_dump, run, small_bin  # noqa: F401  (fixtures)
from tests.test_cluster_cli import final_window

pytestmark = pytest.mark.gpu

K = 64


def parse(stdout, sources):
    """[batch][source] -> (L, edges); asserts the order of the lines."""
    lines = [l.split() for l in stdout.splitlines() if l.startswith("subgraph ")]
    assert len(lines) == BATCHES * len(sources) and all(len(l) == 6 for l in lines), lines[:3]
    assert all(l[2::2] == ["vertices", "edges"] for l in lines)
    assert [int(l[1]) for l in lines] == list(sources) * BATCHES  # batch by batch, in source order
    recs = [(int(l[3]), int(l[5])) for l in lines]
    return [recs[b * len(sources):(b + 1) * len(sources)] for b in range(BATCHES)]


def parse_file(path, sources):
    """source -> (ids, p, rows as (tail, head) pairs in file order); asserts the order of the lines."""
    out = {s: ([], [], []) for s in sources}
    seen = []
    for l in open(path).read().splitlines():
        f = l.split()
        s = int(f[1])
        if not seen or seen[-1] != s:
            seen.append(s)
        if f[0] == "v":
            assert len(f) == 5 and int(f[2]) == len(out[s][0]) and not out[s][2]  # positions in order, the vertices before the edges
            out[s][0].append(int(f[3]))
            out[s][1].append(float(f[4]))
        else:
            assert f[0] == "e" and len(f) == 4
            out[s][2].append((int(f[2]), int(f[3])))
    assert seen == list(sources)
    return out


@pytest.mark.parametrize("n_src", [1, 3])
def test_subgraph_lines_and_file_equal_the_restatement(pagerank, small_bin, tmp_path, n_src):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, n_src)]
    srcf = tmp_path / "sources.txt"
    srcf.write_text("\n".join(map(str, sources)) + "\n")
    args = [pagerank] + base_args(path) + (["-s", str(sources[0])] if n_src == 1 else ["--sources", str(srcf)])
    e, graph = final_window(V, e1, e2)
    graph = graph[:3]
    for name, env in (("serial", SERIAL), ("overlapped", None)):  # (the overlapped loop names the epoch its states stand on)
        dump, outf = str(tmp_path / f"{name}.dump"), str(tmp_path / f"{name}.subgraph")
        r = run(args + ["--dump", dump, "--subgraph", str(K), "--subgraph-out", outf], env_extra=env)
        assert r.returncode == 0, r.stdout
        got = parse(r.stdout, sources)
        if name == "serial":
            shown = r.stdout
        for recs in got:
            assert all(1 < L <= K and m > 0 for L, m in recs), recs
        written = parse_file(outf, sources)
        dumps = read_dump(dump)
        for j, s in enumerate(sources):
            p, res = dumps[s]
            ids = np.nonzero(p > 0.0)[0]
            order = ids[np.lexsort((ids, -p[ids]))[:K]]
            rows = subgraph_ref.rows(*graph, order)
            want_edges = [(t, int(b)) for t, row in enumerate(rows) for b in row]
            assert got[-1][j] == (len(order), len(want_edges)), (name, s, got[-1][j])
            f_ids, f_p, f_edges = written[s]
            assert f_ids == order.tolist() and f_p == p[order].tolist() and f_edges == want_edges, (name, s)
            slot = e.add_source(s)
            e.write(slot, p, res)
            cnt, c_ids, c_p, c_rp, c_col = e.subgraph(slot, K)
            assert cnt == len(order) and c_ids[:cnt].tolist() == f_ids and c_p[:cnt].tolist() == f_p
            assert [(t, int(b)) for t in range(cnt) for b in c_col[c_rp[t]:c_rp[t + 1]]] == f_edges
    e.close()
    # without the flag: no such line, and otherwise the same sequence of lines
    plain = run(args + ["--dump", str(tmp_path / "plain.dump")], env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^subgraph ", plain.stdout, re.M)

    def shape(text):  # (what every line begins with; the child's two streams share one pipe, so the order is not compared)
        return sorted(l.split()[0].split("=")[0] for l in text.splitlines() if l.strip() and not l.startswith("subgraph "))

    assert shape(shown) == shape(plain.stdout)


def test_bad_arguments_are_rejected(pagerank, small_bin, tmp_path):
    path = small_bin[0]
    for extra in (["--subgraph", "0"], ["--subgraph", "-1"], ["--subgraph", "8193"], ["--subgraph-out", str(tmp_path / "x")]):
        r = run([pagerank] + base_args(path) + extra)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and not re.search(r"^subgraph ", r.stdout, re.M), extra
    assert not (tmp_path / "x").exists()
