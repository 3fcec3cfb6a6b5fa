"""./pagerank --cluster K [--cluster-min P] [--cluster-min-size M]: after every batch one line `cluster <source> size <n> cut <c>
vol <v> phi <phi>` per source, through dppr_cluster / dppr_group_cluster. The lines of the last batch equal, exactly (%.17g
round-trips a double), what the binding's dppr_cluster returns for the dumped state on the same window, and the restatement of
tests/cluster_ref.py over that state's order. (Two solves of one stream agree to far below the tolerance, not always to the bit, and
a last bit can swap two vertices of the order: the earlier batches are compared by their shape.) Without the flag stdout has no such
line and is otherwise the same sequence of lines; a bad argument is found before any device work."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import cluster_ref
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args
from tests.test_cli import pagerank, read_dump, run, small_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

K, MIN_P, MIN_SIZE = 64, 1e-7, 3


def parse(stdout, sources):
    """[batch][source] -> dict; asserts the order of the lines."""
    lines = [l.split() for l in stdout.splitlines() if l.startswith("cluster ")]
    assert len(lines) == BATCHES * len(sources) and all(len(l) == 10 for l in lines), lines[:3]
    assert all(l[2::2] == ["size", "cut", "vol", "phi"] for l in lines)
    assert [int(l[1]) for l in lines] == list(sources) * BATCHES  # batch by batch, in source order
    recs = [dict(best_size=int(l[3]), best_cut=int(l[5]), best_vol=int(l[7]), best_phi=float(l[9])) for l in lines]
    return [recs[b * len(sources):(b + 1) * len(sources)] for b in range(BATCHES)]


def final_window(V, e1, e2):
    """The same stream through the binding, to its last window: the engine (epoch = the last batch's) and its graph."""
    g = orc.Graph(V, e1, e2, 0, W, C)
    e = eng.Engine(V, W, 0, C)
    e.load_window(*g.window_edges())
    for _ in range(BATCHES):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
    row, col = e.read_out_graph()
    return e, (V, row, col, len(col))


@pytest.mark.parametrize("n_src", [1, 3])
def test_cluster_lines_equal_the_abi_call(pagerank, small_bin, tmp_path, n_src):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, n_src)]
    srcf = tmp_path / "sources.txt"
    srcf.write_text("\n".join(map(str, sources)) + "\n")
    args = [pagerank] + base_args(path) + (["-s", str(sources[0])] if n_src == 1 else ["--sources", str(srcf)])
    flags = ["--cluster", str(K), "--cluster-min", repr(MIN_P), "--cluster-min-size", str(MIN_SIZE)]
    e, graph = final_window(V, e1, e2)
    for name, env in (("serial", SERIAL), ("overlapped", None)):  # (the overlapped loop names the epoch its states stand on)
        dump = str(tmp_path / f"{name}.dump")
        r = run(args + ["--dump", dump] + flags, env_extra=env)
        assert r.returncode == 0, r.stdout
        got = parse(r.stdout, sources)
        if name == "serial":
            shown = r.stdout
        for recs in got:
            assert all(MIN_SIZE <= b["best_size"] <= K and 0 < b["best_vol"] and 0.0 <= b["best_phi"] <= 1.0 for b in recs), recs
        dumps = read_dump(dump)
        for j, s in enumerate(sources):
            p, res = dumps[s]
            slot = e.add_source(s)
            e.write(slot, p, res)
            ids = np.nonzero(p > MIN_P)[0]
            order = ids[np.lexsort((ids, -p[ids]))[:K]]
            want = cluster_ref.cluster(*graph, order, K, MIN_SIZE)[0]
            call = e.cluster(slot, K, MIN_P, MIN_SIZE)
            assert call["count"] == want["count"] == len(order) > MIN_SIZE
            for rec in (want, call):
                assert got[-1][j] == {k: rec[k] for k in ("best_size", "best_cut", "best_vol", "best_phi")}, (name, s, got[-1][j], rec)
    e.close()
    # without the flag: no such line, and otherwise the same sequence of lines
    plain = run(args + ["--dump", str(tmp_path / "plain.dump")], env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^cluster ", plain.stdout, re.M)

    def shape(text):  # (what every line begins with; the child's two streams share one pipe, so the order is not compared)
        return sorted(l.split()[0].split("=")[0] for l in text.splitlines() if l.strip() and not l.startswith("cluster "))

    assert shape(shown) == shape(plain.stdout)


def test_bad_arguments_are_rejected(pagerank, small_bin):
    path = small_bin[0]
    cases = [["--cluster", "0"], ["--cluster", "-1"], ["--cluster", "8193"], ["--cluster", "64", "--cluster-min", "-1e-3"],
             ["--cluster", "64", "--cluster-min", "nan"], ["--cluster", "64", "--cluster-min-size", "0"],
             ["--cluster", "64", "--cluster-min-size", "65"], ["--cluster-min", "1e-6"], ["--cluster-min-size", "2"]]
    for extra in cases:
        r = run([pagerank] + base_args(path) + extra)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and not re.search(r"^cluster ", r.stdout, re.M), extra
