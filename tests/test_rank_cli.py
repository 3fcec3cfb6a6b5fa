"""./pagerank --topk K --rank-factor none|deg|inv-deg --rank-exclude seeds,in,out: after the topk lines one line
`ranked <source> <rank> <vertex> <score>` per entry, through dppr_topk_ranked / dppr_group_topk_ranked on the newest epoch. The
lines equal, exactly (%.17g round-trips a double), the restatement of tests/rank_ref.py over the state the same run dumped and the
last window's graph read back through the binding; the topk lines are those of a run without the flags, text for text.
That comparison of two runs needs streams on which a solve repeats itself to the bit, the ones tests/test_changes_cli.py rests on:
a source GROUP on the small .bin (its sweeps gather: no sum depends on an arrival order), and for a single source -- whose pushes
add into a vertex from every out-neighbour in whatever order they arrive, so that two runs on the small .bin differ in a last bit --
the stream of one out-edge per vertex, where every vertex receives one addend per iteration."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen
from tests import rank_ref
from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args, one_out_stream
from tests.test_cli import pagerank, read_dump, run, small_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

K = 5


def lines_of(stdout, word, sources):
    """{source: [(vertex, score), ..]} of the `word` lines; asserts source order and ranks from 1."""
    out, order = {}, []
    for l in stdout.splitlines():
        f = l.split()
        if f and f[0] == word:
            assert len(f) == 5, l
            s = int(f[1])
            if s not in out:
                out[s] = []
                order.append(s)
            assert int(f[2]) == len(out[s]) + 1, l
            out[s].append((int(f[3]), float(f[4])))
    assert order == [s for s in sources if s in out]
    return out


def final_graph(V, e1, e2, directed):
    """The out-CSR of the last window by external id: the same stream through the binding."""
    g = orc.Graph(V, e1, e2, directed, W, C)
    e = eng.Engine(V, W, directed, C)
    e.load_window(*g.window_edges())
    for _ in range(BATCHES):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
    row, col = e.read_out_graph()
    e.close()
    return row, col


@pytest.mark.parametrize("n_src,factor,exclude,flags", [(1, "deg", "seeds,in", 3), (3, "deg", "seeds,in", 3), (3, "inv-deg", "out", 4),
                                                        (3, None, "seeds,in,out", 7)])
def test_ranked_lines_equal_the_reference(pagerank, small_bin, tmp_path, n_src, factor, exclude, flags):
    if n_src == 1:  # one out-edge per vertex in window + batch, towards low ids; the source is vertex 0
        directed, sources = 1, [0]
        V, e1, e2 = one_out_stream()
        for lo in range(0, BATCHES * C + 1, C):
            assert len(np.unique(e1[lo:lo + W + C])) == W + C
        path = str(tmp_path / "one_out.bin")
        datagen.write_bin(path, V, e1, e2)
        args = [pagerank] + base_args(path, directed=1) + ["-s", "0"]
    else:
        directed = 0
        path, V, e1, e2 = small_bin
        sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, n_src)]
        srcf = tmp_path / "sources.txt"
        srcf.write_text("\n".join(map(str, sources)) + "\n")
        args = [pagerank] + base_args(path) + ["--sources", str(srcf)]
    dump = str(tmp_path / "ranked.dump")
    rank = (["--rank-factor", factor] if factor else []) + ["--rank-exclude", exclude]  # (either flag alone is enough)
    r = run(args + ["--topk", str(K)] + rank + ["--dump", dump], env_extra=SERIAL)
    assert r.returncode == 0, r.stdout
    plain = run(args + ["--topk", str(K)], env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^ranked ", plain.stdout, re.M)
    topk = [l for l in r.stdout.splitlines() if l.startswith("topk ")]
    assert len(topk) == K * n_src and topk == [l for l in plain.stdout.splitlines() if l.startswith("topk ")]
    row, col = final_graph(V, e1, e2, directed)
    tails, heads = rank_ref.edges(row, col)
    deg = rank_ref.out_degree(V, tails)
    dumps = read_dump(dump)
    cols = [dumps[s][0] for s in sources]
    ex = rank_ref.excluded(V, tails, heads, [[s] for s in sources], flags)
    kind = {None: rank_ref.NONE, "deg": rank_ref.DEG, "inv-deg": rank_ref.INV_DEG}[factor]
    want = rank_ref.scores(cols, kind, outdeg=deg, excl=ex)
    got = lines_of(r.stdout, "ranked", sources)
    shown = lines_of(r.stdout, "topk", sources)
    for i, s in enumerate(sources):
        wi, ws = rank_ref.topk(want[i], K)
        assert len(wi) == K and got[s] == list(zip(wi.tolist(), ws.tolist())), (s, got[s], wi, ws)
        pi, pp = rank_ref.topk(cols[i], K)
        assert shown[s] == list(zip(pi.tolist(), pp.tolist()))
        if flags & 1:
            assert shown[s][0][0] == s and s not in [v for v, _ in got[s]]
