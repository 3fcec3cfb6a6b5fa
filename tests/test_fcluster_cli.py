"""./pagerank --forward-track FILE --push-eps E --forward-cluster deg|p: one `fcluster` line per set of FILE after the create and after
every batch, `fcluster <first id> size <best_size> of <count> cut <cut_out> vol <vol> phi <%.17g>`, through dppr_ftrack_cluster. The
lines equal the numpy definition of tests/fcluster_ref.py over the track of tests/ftrack_ref.py batch by batch -- the integers integer
for integer, phi to its 17 digits --, under both orders; the loop that builds the next graph beside the solve prints the same lines.
Without the flag stdout has no such line; bad arguments are refused with the usage before any device work."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import fcluster_ref as fcr
from tests import ftrack_ref as tr
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args
from tests.test_cli import pagerank, run, small_bin  # noqa: F401  (fixtures)
from tests.test_forward_gpu import rows_of

pytestmark = pytest.mark.gpu

EPS, ROUNDS = 1e-5, 12


def parse(stdout, sets):
    """[[(first id, best_size, count, cut, vol, phi)] per block]: the create, then every batch."""
    lines = [l.split() for l in stdout.splitlines() if l.startswith("fcluster ")]
    assert len(lines) == (BATCHES + 1) * len(sets), len(lines)
    out = []
    for b in range(BATCHES + 1):
        block = []
        for i, (ids, _) in enumerate(sets):
            f = lines[b * len(sets) + i]
            assert f[0::2] == ["fcluster", "size", "of", "cut", "vol", "phi"] and int(f[1]) == ids[0], f
            block.append((int(f[1]), int(f[3]), int(f[5]), int(f[7]), int(f[9]), float(f[11])))
        out.append(block)
    return out


def reference(V, e1, e2, sources, sets, order, directed=0):
    """The same stream through numpy; the rows of every epoch are read from an engine fed as the binding feeds it."""
    g = orc.Graph(V, e1, e2, directed, W, C)
    e = eng.Engine(V, W, directed, C, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    cols = [tr.Column(rows_of(e), ids, w, EPS, ROUNDS) for ids, w in sets]

    def block():
        row, col = e.read_out_graph()
        out = []
        for (ids, _), c in zip(sets, cols):
            b = fcr.cluster(c.p, row, col, order)[0]
            out.append((int(ids[0]), b["best_size"], b["count"], b["best_cut"], b["best_vol"], b["best_phi"]))
        return out

    ref = [block()]
    for _ in range(BATCHES):
        assert not g.stream_updates()
        g.inc_construct(1)
        rec = g.batch()
        e.set_batch(*rec)
        e.slide(*g.new_stream())
        rows = rows_of(e)
        for c in cols:
            c.update(rows, rec, ROUNDS)
        ref.append(block())
    e.close()
    return ref


def test_fcluster_lines_equal_numpy(pagerank, small_bin, tmp_path):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, 3)]
    named = np.unique(np.concatenate([e1[:W], e2[:W]]))
    never = np.setdiff1d(np.arange(V), np.unique(np.concatenate([e1, e2])))
    sets = [(np.array([s]), np.ones(1)) for s in sources + [int(x) for x in named[::len(named) // 12][:12]] + [int(never[0])]]
    sets.append((np.array([sources[0], int(never[0]), int(named[3])]), np.array([0.25, 1.5, 3.0])))
    sets.append((named[5:45].astype(np.int64), 0.5 + np.arange(40) / 64.0))
    assert len(sets) == 18   # two tracks: 16 + 2
    sf, pf = tmp_path / "sources.txt", tmp_path / "track.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    pf.write_text("".join(" ".join(f"{int(i)}" if x == 1.0 else f"{int(i)}:{float(x)!r}" for i, x in zip(ids, w)) + "\n" for ids, w in sets))
    flags = ["--forward-track", str(pf), "--push-eps", str(EPS), "--push-rounds", str(ROUNDS)]
    args = [pagerank] + base_args(path) + ["--sources", str(sf)]
    for order in ("deg", "p"):
        r = run(args + flags + ["--forward-cluster", order], env_extra=SERIAL)
        assert r.returncode == 0, r.stdout[-2000:]
        got = parse(r.stdout, sets)
        assert got == reference(V, e1, e2, sources, sets, order), order
        assert got[-1][15][1:] == (0, 0, 0, 0, float("inf"))   # a vertex the stream never names: an empty order
        assert any(b[2] > 100 for b in got[-1]) and len(re.findall(r"^ftrack ", r.stdout, re.M)) == len(got) * len(sets)
    beside = run(args + flags + ["--forward-cluster", "p"])   # the default loop: the next graph is built beside the solve
    assert beside.returncode == 0 and parse(beside.stdout, sets) == got, beside.stdout[-2000:]
    plain = run(args + flags, env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^fcluster ", plain.stdout, re.M)
    for bad in (["--forward-cluster", "deg"], flags + ["--forward-cluster", "degree"], flags + ["--forward-cluster", ""]):
        x = run(args + bad)
        assert x.returncode != 0 and "invalid arguments" in x.stdout and "--forward-cluster deg|p" in x.stdout, (bad, x.stdout[-400:])
        assert "fcluster " not in x.stdout.split("invalid arguments")[0], bad
