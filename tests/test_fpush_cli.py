"""./pagerank --forward-push FILE --push-eps E [--push-rounds N] [--forward-topk K]: after every batch one line per set of FILE,
`fpush <first id> seeds <n> rounds <used> converged <0|1> rem <mass> pushes <n> left <n> top <found> <v0>:<p0> ...`, through
dppr_forward_push on the epoch the states stand on. The lines equal what Engine.forward_push gives on the same stream driven through
the Python binding -- the integers integer for integer, rem and p to their 17 digits --, batch by batch, and the last batch equals the
numpy restatement of tests/fpush_ref.py. 18 sets go in two calls (16 + 2). Without the flag stdout has no such line."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import forward_ref as fr
from tests import fpush_ref as pr
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args
from tests.test_cli import pagerank, run, small_bin  # noqa: F401  (fixtures)
from tests.test_forward_gpu import rows_of

pytestmark = pytest.mark.gpu

EPS, ROUNDS, TOPK = 1e-5, 12, 6
NAMES = ["fpush", "seeds", "rounds", "converged", "rem", "pushes", "left", "top"]


def parse(stdout, sets):
    """[[(first id, seeds, rounds, converged, rem, pushes, left, [(id, p)])] per batch]; asserts the order of the lines."""
    lines = [l.split() for l in stdout.splitlines() if l.startswith("fpush ")]
    assert len(lines) == BATCHES * len(sets), len(lines)
    out = []
    for b in range(BATCHES):
        block = []
        for i, (ids, _) in enumerate(sets):
            f = lines[b * len(sets) + i]
            assert f[0:16:2] == NAMES and int(f[1]) == ids[0] and int(f[3]) == len(ids), f
            pairs = [(int(x.split(":")[0]), float(x.split(":")[1])) for x in f[16:]]
            assert len(pairs) == int(f[15]), f
            block.append((int(f[1]), int(f[3]), int(f[5]), int(f[7]), float(f[9]), int(f[11]), int(f[13]), pairs))
        out.append(block)
    return out


def feed(V, e1, e2, sources, sets, directed=0):
    """The same stream through the binding: the calls of 16 sets per batch; the last batch also through numpy."""
    g = orc.Graph(V, e1, e2, directed, W, C)
    e = eng.Engine(V, W, directed, C, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    h = e.add_source_group(sources)
    e.group_init_solve(h, 1e-9)
    out = []
    for _ in range(BATCHES):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.group_update(h, 1e-9)
        block = []
        for first in range(0, len(sets), 16):
            part = sets[first:first + 16]
            got = e.forward_push(part, EPS, ROUNDS, k=TOPK)
            for j, (ids, _) in enumerate(part):
                tid, tp = got["topk"][j]
                block.append((int(ids[0]), len(ids), int(got["rounds_used"][j]), int(got["converged"][j]), float(got["rem"][j]),
                              int(got["pushes"][j]), int(got["left"][j]), list(zip(tid.tolist(), tp.tolist()))))
        out.append(block)
    rows = rows_of(e)
    rowless = pr.rowless_mask(rows)
    numpy_last = []
    for ids, w in sets:
        c = pr.push(rows, rowless, ids, w, EPS, ROUNDS)
        tid, tp = fr.topk(c.p, TOPK)
        numpy_last.append((int(ids[0]), len(ids), c.rounds_used, c.converged, c.rem, c.pushes, c.left, list(zip(tid.tolist(), tp.tolist()))))
    e.close()
    return out, numpy_last


def test_fpush_lines_equal_the_binding_and_numpy(pagerank, small_bin, tmp_path):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, 3)]
    named = np.unique(np.concatenate([e1[:W], e2[:W]]))
    never = np.setdiff1d(np.arange(V), np.unique(np.concatenate([e1, e2])))
    sets = [(np.array([s]), np.ones(1)) for s in sources + [int(x) for x in named[::len(named) // 12][:12]] + [int(never[0])]]
    sets.append((np.array([sources[0], int(never[0]), int(named[3])]), np.array([0.25, 1.5, 3.0])))
    sets.append((named[5:45].astype(np.int64), 0.5 + np.arange(40) / 64.0))
    assert len(sets) == 18
    sf, pf = tmp_path / "sources.txt", tmp_path / "push.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    pf.write_text("".join(" ".join(f"{int(i)}" if x == 1.0 else f"{int(i)}:{float(x)!r}" for i, x in zip(ids, w)) + "\n" for ids, w in sets))
    flags = ["--forward-push", str(pf), "--push-eps", str(EPS), "--push-rounds", str(ROUNDS), "--forward-topk", str(TOPK)]
    args = [pagerank] + base_args(path) + ["--sources", str(sf)]
    r = run(args + flags, env_extra=SERIAL)
    assert r.returncode == 0, r.stdout[-2000:]
    got = parse(r.stdout, sets)
    want, numpy_last = feed(V, e1, e2, sources, sets)
    assert got == want
    assert got[-1] == numpy_last
    last = got[-1]
    assert last[15][2:] == (0, 1, 0.0, 0, 0, [(int(never[0]), 0.15)])                  # a vertex the stream never names
    assert any(b[3] == 0 for b in last) and all(b[4] >= 0.0 and (b[6] == 0) == (b[3] == 1) for b in last)
    assert all(len(b[7]) <= TOPK and all(x[1] >= y[1] for x, y in zip(b[7], b[7][1:])) for b in last)
    beside = run(args + flags)  # the default loop: the next graph is built beside the solve
    assert beside.returncode == 0 and parse(beside.stdout, sets) == got, beside.stdout[-2000:]
    # the default cap on the rounds, and --forward-topk 0: no vertex follows the count
    dflt = run(args + ["--forward-push", str(pf), "--push-eps", "1e-4", "--forward-topk", "0"], env_extra=SERIAL)
    assert dflt.returncode == 0
    lines = [l.split() for l in dflt.stdout.splitlines() if l.startswith("fpush ")]
    assert len(lines) == BATCHES * 18 and all(len(l) == 16 and l[15] == "0" for l in lines)
    # without the flag: no such line
    plain = run(args, env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^fpush ", plain.stdout, re.M)
