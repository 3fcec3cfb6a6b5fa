"""./pagerank --changes K [--changes-min D]: after every batch, per source in source order, one line `moved <batch> <source>
<count>` and up to K lines `changes <batch> <source> <rank> <vertex> <delta> <pagerank>`, through dppr_changes /
dppr_group_changes with remark = 1 (the per-batch feed). The lines agree with the same stream driven through the Python binding:
ids equal, values equal after the %.17g round trip.

Two solves of one stream can only be compared bit for bit where the solver itself is reproducible. A source group is, on the
synchronous schedule (its sweeps gather). The single-source solver pushes with float atomics, and two pushes that reach one
residual in the same iteration add in arrival order (tests/test_cli.py holds two such runs to 1e-14, not to the bit). The slot
run therefore streams a graph in which every vertex has at most ONE out-edge in any window plus batch (one_out_stream): a
reverse push at u adds to the tails of u's in-edges, so every residual receives at most one add per synchronous iteration,
every batch has at most one record per tail, and the solve is the same to the bit whatever the arrival order. Both sides run
the synchronous schedule and ./pagerank its serial batch loop (DPPR_NO_OVERLAP=1: the binding's call sequence); the default,
overlapped loop is run as well. Without the flag stdout has no such line."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests.test_cli import pagerank, run, small_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

K = 5
SERIAL = {"DPPR_NO_OVERLAP": "1"}   # ./pagerank's serial batch loop: the call sequence of the binding
W, C, BATCHES = 600, 6, 4   # what -w 0.1 -n 0 -r 0.01 -b 4 derive from the 6000 edges of small_bin


def base_args(path, directed=0):
    return ["-d", path, "-a", "0", "-i", str(directed), "-y", "1", "-n", "0", "-r", "0.01", "-b", str(BATCHES), "--sync"]


def one_out_stream(V=1024, n=6000, period=1000, seed=5):
    """A directed stream whose tails cycle with a period above W + C: in any window plus batch every vertex is the tail of at
    most one edge. Heads lie below their tail (30 % of them are vertex 0, the source), so the edges form trees towards low ids."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) % period
    h = rng.integers(0, t // 2 + 1)
    h[rng.random(n) < 0.3] = 0
    h[h == t] = (t[h == t] + 1) % period
    return V, t.astype(np.int32), h.astype(np.int32)


def parse(stdout, sources):
    """{(batch, source): (moved, [(rank, vertex, delta, p), ..])}; asserts the order of the lines."""
    out, order = {}, []
    for l in stdout.splitlines():
        f = l.split()
        if l.startswith("moved "):
            assert len(f) == 4, l
            key = (int(f[1]), int(f[2]))
            assert key not in out, l
            out[key] = (int(f[3]), [])
            order.append(key)
        elif l.startswith("changes "):
            assert len(f) == 7, l
            key = (int(f[1]), int(f[2]))
            assert order and order[-1] == key, l  # the entries of a source follow its `moved` line
            out[key][1].append((int(f[3]), int(f[4]), float(f[5]), float(f[6])))
    assert order == [(b, s) for b in range(1, BATCHES + 1) for s in sources]  # batch by batch, in source order
    for moved, lines in out.values():
        assert [r for r, _, _, _ in lines] == list(range(1, min(moved, K) + 1))
        mags = [abs(d) for _, _, d, _ in lines]
        assert all(a > b or (a == b and u < v) for a, b, u, v in zip(mags, mags[1:], [x[1] for x in lines], [x[1] for x in lines[1:]]))
    return out


def feed(V, e1, e2, sources, as_group, min_delta=0.0, directed=0):
    """The same stream through the binding: mark after the from-scratch solve, one query with remark=True per batch."""
    g = orc.Graph(V, e1, e2, directed, W, C)
    e = eng.Engine(V, W, directed, C, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    h = e.add_source_group(sources) if as_group else e.add_source(sources[0])
    if as_group:
        e.group_init_solve(h, 1e-9)
        e.group_mark(h)
    else:
        e.init_solve(h, 1e-9)
        e.mark(h)
    out = {}
    for b in range(1, BATCHES + 1):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        if as_group:
            e.group_update(h, 1e-9)
            res = e.group_changes(h, K, min_delta, remark=True)
        else:
            e.update(h, 1e-9)
            res = [e.changes(h, K, min_delta, remark=True)]
        for s, (ids, d, p, moved) in zip(sources, res):
            out[(b, s)] = (moved, [(t + 1, int(ids[t]), float(d[t]), float(p[t])) for t in range(len(ids))])
    e.close()
    return out


def test_one_source(pagerank, tmp_path):
    V, e1, e2 = one_out_stream()
    for lo in range(0, BATCHES * C + 1, C):  # the property the bit comparison rests on: one out-edge per vertex in window + batch
        assert len(np.unique(e1[lo:lo + W + C])) == W + C
    path = str(tmp_path / "one_out.bin")
    datagen.write_bin(path, V, e1, e2)
    src = 0
    args = base_args(path, directed=1) + ["-s", str(src)]
    r = run([pagerank] + args + ["--changes", str(K)], env_extra=SERIAL)
    assert r.returncode == 0, r.stdout
    got = parse(r.stdout, [src])
    assert all(moved > K and len(lines) == K for moved, lines in got.values())
    assert any(d > 0 for _, lines in got.values() for _, _, d, _ in lines) and any(d < 0 for _, lines in got.values() for _, _, d, _ in lines)
    assert got == feed(V, e1, e2, [src], as_group=False, directed=1)  # (%.17g round-trips a double)
    beside = run([pagerank] + args + ["--changes", str(K)])  # the default loop: the next graph is built beside the solve
    assert beside.returncode == 0, beside.stdout
    assert parse(beside.stdout, [src]) == got
    plain = run([pagerank] + args, env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^(changes|moved) ", plain.stdout, re.M)
    # what the timed region reports does not depend on the flag: the same lines, in the same number
    keys = r"^(coming stream_batch_count=\d+|edge_num \d+)$"
    assert re.findall(keys, r.stdout, re.M) == re.findall(keys, plain.stdout, re.M)


def test_sources_file_as_a_group(pagerank, small_bin, tmp_path):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, 5)]
    sf = tmp_path / "sources.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    r = run([pagerank] + base_args(path) + ["--sources", str(sf), "--changes", str(K), "--changes-min", "1e-7"], env_extra=SERIAL)
    assert r.returncode == 0, r.stdout
    got = parse(r.stdout, sources)
    assert got == feed(V, e1, e2, sources, as_group=True, min_delta=1e-7)
    assert all(abs(d) > 1e-7 for _, lines in got.values() for _, _, d, _ in lines)
    plain = run([pagerank] + base_args(path) + ["--sources", str(sf)])
    assert plain.returncode == 0 and not re.search(r"^(changes|moved) ", plain.stdout, re.M)


def test_bad_values_are_rejected(pagerank, small_bin):
    for bad in (["--changes", "8193"], ["--changes", "-1"], ["--changes", "5", "--changes-min", "-1"], ["--changes-min", "0.5"]):
        r = run([pagerank] + base_args(small_bin[0]) + bad)
        assert r.returncode != 0 and "invalid arguments" in r.stdout, bad
