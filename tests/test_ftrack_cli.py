"""./pagerank --forward-track FILE --push-eps E [--push-rounds N] [--forward-topk K]: one `ftrack` line per set of FILE after the initial
solve (the create) and after every batch (the update), `ftrack <first id> seeds <n> epoch <e> rounds <used> converged <0|1> rem <fold
of |r|> pushes <n> fix <records> <tails> <heads> top <found> <v0>:<p0> ...`, through dppr_ftrack_create / dppr_ftrack_update. The lines
equal what Engine.ftrack gives on the same stream driven through the Python binding -- the integers integer for integer, rem and p
to their 17 digits --, and the numpy definition of tests/ftrack_ref.py batch by batch. 18 sets go in two tracks (16 + 2). The loop
that builds the next graph beside the solve prints the same lines. Without the flag stdout has no such line; bad arguments are
refused with the usage before any device work."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import forward_ref as fr
from tests import ftrack_ref as tr
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args
from tests.test_cli import pagerank, run, small_bin  # noqa: F401  (fixtures)
from tests.test_forward_gpu import rows_of

pytestmark = pytest.mark.gpu

EPS, ROUNDS, TOPK = 1e-5, 12, 6
NAMES = ["ftrack", "seeds", "epoch", "rounds", "converged", "rem", "pushes"]


def parse(stdout, sets):
    """[[(first id, seeds, epoch, rounds, converged, rem, pushes, fix, [(id, p)])] per block]: the create, then every batch."""
    lines = [l.split() for l in stdout.splitlines() if l.startswith("ftrack ")]
    assert len(lines) == (BATCHES + 1) * len(sets), len(lines)
    out = []
    for b in range(BATCHES + 1):
        block = []
        for i, (ids, _) in enumerate(sets):
            f = lines[b * len(sets) + i]
            assert f[0:14:2] == NAMES and f[14] == "fix" and f[18] == "top" and int(f[1]) == ids[0] and int(f[3]) == len(ids), f
            pairs = [(int(x.split(":")[0]), float(x.split(":")[1])) for x in f[20:]]
            assert len(pairs) == int(f[19]), f
            block.append((int(f[1]), int(f[3]), int(f[5]), int(f[7]), int(f[9]), float(f[11]), int(f[13]), [int(x) for x in f[15:18]], pairs))
        out.append(block)
    return out


def feed(V, e1, e2, sources, sets, directed=0):
    """The same stream through the binding (tracks of 16 sets) and through numpy."""
    g = orc.Graph(V, e1, e2, directed, W, C)
    e = eng.Engine(V, W, directed, C, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    h = e.add_source_group(sources)
    e.group_init_solve(h, 1e-9)
    parts = [sets[first:first + 16] for first in range(0, len(sets), 16)]
    rows = rows_of(e)
    cols = [tr.Column(rows, ids, w, EPS, ROUNDS) for ids, w in sets]
    tracks = [e.ftrack(part, EPS, ROUNDS, k=TOPK) for part in parts]

    def block(results, epoch):
        out = []
        for part, got in zip(parts, results):
            for j, (ids, _) in enumerate(part):
                tid, tp = got["topk"][j]
                out.append((int(ids[0]), len(ids), epoch, int(got["rounds_used"][j]), int(got["converged"][j]), float(got["rem"][j]),
                            int(got["pushes"][j]), got["fix"].tolist(), list(zip(tid.tolist(), tp.tolist()))))
        return out

    def numpy_block(epoch):
        out = []
        for (ids, _), c in zip(sets, cols):
            tid, tp = fr.topk(c.p, TOPK)
            out.append((int(ids[0]), len(ids), epoch, c.last.rounds_used, c.last.converged, c.last.rem, c.last.pushes, c.last.fix,
                        list(zip(tid.tolist(), tp.tolist()))))
        return out

    out, ref = [block([t.created for t in tracks], 0)], [numpy_block(0)]
    for _ in range(BATCHES):
        assert not g.stream_updates()
        g.inc_construct(1)
        rec = g.batch()
        e.set_batch(*rec)
        ep = e.slide(*g.new_stream())
        e.group_update(h, 1e-9)
        out.append(block([t.update(ep, ROUNDS, k=TOPK) for t in tracks], ep))
        rows = rows_of(e)
        for c in cols:
            c.update(rows, rec, ROUNDS)
        ref.append(numpy_block(ep))
    e.close()
    return out, ref


def test_ftrack_lines_equal_the_binding_and_numpy(pagerank, small_bin, tmp_path):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, 3)]
    named = np.unique(np.concatenate([e1[:W], e2[:W]]))
    never = np.setdiff1d(np.arange(V), np.unique(np.concatenate([e1, e2])))
    sets = [(np.array([s]), np.ones(1)) for s in sources + [int(x) for x in named[::len(named) // 12][:12]] + [int(never[0])]]
    sets.append((np.array([sources[0], int(never[0]), int(named[3])]), np.array([0.25, 1.5, 3.0])))
    sets.append((named[5:45].astype(np.int64), 0.5 + np.arange(40) / 64.0))
    assert len(sets) == 18
    sf, pf = tmp_path / "sources.txt", tmp_path / "track.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    pf.write_text("".join(" ".join(f"{int(i)}" if x == 1.0 else f"{int(i)}:{float(x)!r}" for i, x in zip(ids, w)) + "\n" for ids, w in sets))
    flags = ["--forward-track", str(pf), "--push-eps", str(EPS), "--push-rounds", str(ROUNDS), "--forward-topk", str(TOPK)]
    args = [pagerank] + base_args(path) + ["--sources", str(sf)]
    r = run(args + flags, env_extra=SERIAL)
    assert r.returncode == 0, r.stdout[-2000:]
    got = parse(r.stdout, sets)
    want, ref = feed(V, e1, e2, sources, sets)
    assert got == want
    assert got == ref
    assert [b[0][2] for b in got] == list(range(BATCHES + 1)) and got[0][0][7] == [0, 0, 0] and all(b[0][7][0] == 4 * C for b in got[1:])
    last = got[-1]
    assert last[15][3:7] == (0, 1, 0.0, 0) and last[15][8] == [(int(never[0]), 0.15)]     # a vertex the stream never names
    assert all(len(b[8]) <= TOPK and all(x[1] >= y[1] for x, y in zip(b[8], b[8][1:])) for b in last)
    beside = run(args + flags)  # the default loop: the next graph is built beside the solve
    assert beside.returncode == 0 and parse(beside.stdout, sets) == got, beside.stdout[-2000:]
    # without the flag: no such line
    plain = run(args, env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^ftrack ", plain.stdout, re.M)
    # refused with the usage, before any device work
    empty = tmp_path / "empty.txt"
    empty.write_text("")
    many = tmp_path / "many.txt"
    many.write_text("".join(f"{int(named[i % len(named)])}\n" for i in range(257)))
    ok = flags[:4]
    for bad in (["--forward-track", str(tmp_path / "missing.txt"), "--push-eps", "1e-5"], ["--forward-track", str(empty), "--push-eps", "1e-5"],
                ["--forward-track", str(many), "--push-eps", "1e-5"], ["--forward-track", str(pf)], ok[:2] + ["--push-eps", "0"],
                ok[:2] + ["--push-eps", "nan"], ok + ["--push-rounds", "0"], ok + ["--push-rounds", "257"], ok + ["--forward-topk", "65"],
                ok + ["--split"]):
        x = run(args + bad)
        assert x.returncode != 0 and "invalid arguments" in x.stdout and "--forward-track <file>" in x.stdout, (bad, x.stdout[-400:])
        assert "ftrack " not in x.stdout.split("invalid arguments")[0], bad
