"""./pagerank --explain FILE [--explain-top F] [--explain-depth D]: after every batch, per source in source order and per id of FILE,
one line `explain <source> <vertex> <end> <len> <v0> <v1> ...` and one line `because <source> <vertex> <w> <mult> <c %.17g>` per
listed contributor, through dppr_explain_at / dppr_group_explain_at on the epoch the states stand on. The lines equal what
Engine.explain_at / Engine.group_explain_at give on the same stream driven through the Python binding, value for value (%.17g
round-trips a double), batch by batch.
That comparison of two solves holds DOUBLES (c, and through it p) to the bit, so it needs streams and loops on which a solve
repeats itself to the bit: exactly the ones tests/test_changes_cli.py rests on and has established. A source GROUP on the small
.bin under the synchronous schedule (its sweeps gather) in ./pagerank's SERIAL batch loop, which is the binding's call sequence;
and a single source on the stream of one out-edge per vertex, where every residual receives at most one add per iteration and
every sum of the invariant has one term, so the solve is the same to the bit whatever the order of arrival: that one is run in
the serial loop and in the default, overlapped loop as well. A group's solve in the overlapped loop is NOT among the premises --
nothing in the project holds it to the bit of the serial one (tests/test_position_cli.py compares integers there) -- so no
comparison of doubles rests on it here. Without the flag stdout has no such line."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args, one_out_stream
from tests.test_cli import pagerank, run, small_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def parse(stdout, sources, ids):
    """[{source: [(end, len, path, [(w, mult, c)]) per id]} per batch]; asserts the order of the lines."""
    lines = [l.split() for l in stdout.splitlines() if l.startswith(("explain ", "because "))]
    out, at = [], 0
    for b in range(BATCHES):
        block = {}
        for s in sources:
            per = []
            for v in ids:
                f = lines[at]
                at += 1
                assert f[0] == "explain" and int(f[1]) == s and int(f[2]) == v and len(f) == 5 + int(f[4]), f
                why = []
                while at < len(lines) and lines[at][0] == "because":
                    w = lines[at]
                    at += 1
                    assert len(w) == 6 and int(w[1]) == s and int(w[2]) == v, w
                    why.append((int(w[3]), int(w[4]), float(w[5])))
                per.append((int(f[3]), int(f[4]), [int(x) for x in f[5:]], why))
            block[s] = per
        out.append(block)
    assert at == len(lines)
    return out


def as_lines(res, i, n_ids):
    """One lane of a binding result in the form of parse()."""
    per = []
    for j in range(n_ids):
        n, k = int(res["len"][j, i]), int(res["nbr_count"][j, i])
        per.append((int(res["end"][j, i]), n, res["path"][j, i, :n].tolist(),
                    [(int(res["nbr"][j, i, t]), int(res["nbr_mult"][j, i, t]), float(res["nbr_c"][j, i, t])) for t in range(k)]))
    return per


def feed(V, e1, e2, sources, ids, as_group, f, depth, directed):
    """The same stream through the binding: one query per batch."""
    g = orc.Graph(V, e1, e2, directed, W, C)
    e = eng.Engine(V, W, directed, C, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    h = e.add_source_group(sources) if as_group else e.add_source(sources[0])
    (e.group_init_solve if as_group else e.init_solve)(h, 1e-9)
    out = []
    for _ in range(BATCHES):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        if as_group:
            e.group_update(h, 1e-9)
            res = e.group_explain_at(h, ids, f, depth)
        else:
            e.update(h, 1e-9)
            res = {k: (v if k in ("deg", "distinct") else v[:, None]) for k, v in e.explain_at(h, ids, f, depth).items()}
        out.append({s: as_lines(res, i, len(ids)) for i, s in enumerate(sources)})
    e.close()
    return out


def ids_file(tmp_path, V, sources):
    rng = np.random.default_rng(9)
    ids = list(sources) + rng.integers(0, V, 40).tolist() + [sources[0], V - 1, 0]   # (a source twice: a duplicate id)
    f = tmp_path / "ids.txt"
    f.write_text("\n".join(map(str, ids)) + "\n")
    return str(f), ids


@pytest.mark.parametrize("opts,f,depth", [([], 3, 16), (["--explain-top", "16", "--explain-depth", "2"], 16, 2),
                                           (["--explain-top", "0", "--explain-depth", "64"], 0, 64)])
def test_sources_file_as_a_group(pagerank, small_bin, tmp_path, opts, f, depth):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, 3)]
    sf = tmp_path / "sources.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    idf, ids = ids_file(tmp_path, V, sources)
    args = [pagerank] + base_args(path) + ["--sources", str(sf), "--explain", idf] + opts
    r = run(args, env_extra=SERIAL)
    assert r.returncode == 0, r.stdout
    got = parse(r.stdout, sources, ids)
    assert got == feed(V, e1, e2, sources, ids, True, f, depth, 0)
    last = got[-1]
    for i, s in enumerate(sources):
        assert last[s][i][:3] == (eng.END_SEED, 1, [s])                         # the source itself: its own seed
        assert last[s][0] == last[s][len(sources) + 40]                         # the duplicate id: the same answer
        assert all(len(why) <= f and n <= depth + 1 for _, n, _, why in last[s])
    assert any(n > 1 for s in sources for _, n, _, _ in last[s])
    if not opts:
        assert any(why for s in sources for _, _, _, why in last[s])
        plain = run([pagerank] + base_args(path) + ["--sources", str(sf)], env_extra=SERIAL)
        assert plain.returncode == 0 and not re.search(r"^(explain|because) ", plain.stdout, re.M)


def test_one_source(pagerank, tmp_path):
    V, e1, e2 = one_out_stream()
    for lo in range(0, BATCHES * C + 1, C):  # the property the comparison rests on: one out-edge per vertex in window + batch
        assert len(np.unique(e1[lo:lo + W + C])) == W + C
    path = str(tmp_path / "one_out.bin")
    datagen.write_bin(path, V, e1, e2)
    idf, ids = ids_file(tmp_path, V, [0])
    args = [pagerank] + base_args(path, directed=1) + ["-s", "0", "--explain", idf, "--explain-top", "2"]
    r = run(args, env_extra=SERIAL)
    assert r.returncode == 0, r.stdout
    got = parse(r.stdout, [0], ids)
    assert got == feed(V, e1, e2, [0], ids, False, 2, 16, 1)
    assert any(n > 2 for blk in got for _, n, _, _ in blk[0]) and any(why for blk in got for _, _, _, why in blk[0])
    beside = run(args)  # the default loop: the next graph is built beside the solve
    assert beside.returncode == 0 and parse(beside.stdout, [0], ids) == got, beside.stdout[-2000:]
    assert all(len(why) <= 1 for blk in got for _, _, _, why in blk[0])   # one out-edge per vertex: one contributor at the most
