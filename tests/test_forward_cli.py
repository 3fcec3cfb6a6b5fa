"""./pagerank --forward FILE [--forward-iters N] [--forward-tol T] [--forward-topk K]: after every batch one line per start of FILE,
`forward <vertex> iters <used> rem <mass remaining> top <found> <v0>:<f0> ...`, through dppr_forward on the epoch the states
stand on. The lines equal what Engine.forward gives on the same stream driven through the Python binding -- the ids integer for
integer, rem and f to their 17 digits --, batch by batch: the sweep reads the graph alone, so no solve has to repeat itself. 20
starts go in two calls (16 + 4). ./pagerank runs its serial batch loop (the binding's call sequence) and, once, the default
overlapped one. Without the flag stdout has no such line, and the lines of the other flags are what they were."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args
from tests.test_cli import pagerank, run, small_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ITERS, TOL, TOPK = 40, 1e-7, 6


def parse(stdout, starts):
    """[[(vertex, used, rem, [(id, f)])] per batch]; asserts the order of the lines."""
    lines = [l.split() for l in stdout.splitlines() if l.startswith("forward ")]
    assert len(lines) == BATCHES * len(starts), len(lines)
    out = []
    for b in range(BATCHES):
        block = []
        for i, s in enumerate(starts):
            f = lines[b * len(starts) + i]
            assert [f[0], f[2], f[4], f[6]] == ["forward", "iters", "rem", "top"] and int(f[1]) == s, f
            pairs = [(int(x.split(":")[0]), float(x.split(":")[1])) for x in f[8:]]
            assert len(pairs) == int(f[7]), f
            block.append((s, int(f[3]), float(f[5]), pairs))
        out.append(block)
    return out


def feed(V, e1, e2, starts, directed=0):
    """The same stream through the binding: the calls of 16 starts per batch."""
    g = orc.Graph(V, e1, e2, directed, W, C)
    e = eng.Engine(V, W, directed, C, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    h = e.add_source_group([int(starts[0]), int(starts[1]), int(starts[2])])
    e.group_init_solve(h, 1e-9)
    out = []
    for _ in range(BATCHES):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.group_update(h, 1e-9)
        block = []
        for first in range(0, len(starts), 16):
            part = starts[first:first + 16]
            got = e.forward(part, ITERS, TOL, k=TOPK)
            for j, s in enumerate(part):
                ids, f = got["topk"][j]
                block.append((int(s), int(got["iters_used"][j]), float(got["rem"][j]), list(zip(ids.tolist(), f.tolist()))))
        out.append(block)
    e.close()
    return out


def test_forward_lines_equal_the_binding(pagerank, small_bin, tmp_path):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, 3)]
    named = np.unique(np.concatenate([e1[:W], e2[:W]]))
    never = np.setdiff1d(np.arange(V), np.unique(np.concatenate([e1, e2])))
    starts = sources + [int(x) for x in named[::len(named) // 15][:15]] + [int(never[0]), sources[0]]
    assert len(starts) == 20
    sf, ff = tmp_path / "sources.txt", tmp_path / "forward.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    ff.write_text("\n".join(map(str, starts)) + "\n")
    flags = ["--forward", str(ff), "--forward-iters", str(ITERS), "--forward-tol", str(TOL), "--forward-topk", str(TOPK)]
    args = [pagerank] + base_args(path) + ["--sources", str(sf)]
    r = run(args + flags, env_extra=SERIAL)
    assert r.returncode == 0, r.stdout[-2000:]
    got = parse(r.stdout, starts)
    assert got == feed(V, e1, e2, starts)
    last = got[-1]
    assert last[18] == (int(never[0]), 8, 0.0, [(int(never[0]), 0.15)])                # a vertex the stream never names
    assert last[19][1:] == last[0][1:] and last[0][3][0][0] == sources[0]              # a repeated start, and it reaches itself most
    assert all(len(b[3]) <= TOPK and all(x[1] >= y[1] for x, y in zip(b[3], b[3][1:])) for b in last)
    assert any(b[1] < ITERS for b in last) and all(0.0 <= b[2] for b in last)
    beside = run(args + flags)  # the default loop: the next graph is built beside the solve
    assert beside.returncode == 0 and parse(beside.stdout, starts) == got, beside.stdout[-2000:]
    # the defaults, and --forward-topk 0: no vertex follows the count
    dflt = run(args + ["--forward", str(ff), "--forward-topk", "0"], env_extra=SERIAL)
    assert dflt.returncode == 0
    lines = [l.split() for l in dflt.stdout.splitlines() if l.startswith("forward ")]
    assert len(lines) == BATCHES * 20 and all(len(l) == 8 and l[7] == "0" for l in lines)
    # without the flag: no such line, and every other line of stdout that holds no time is what it was
    plain = run(args, env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^forward ", plain.stdout, re.M)
