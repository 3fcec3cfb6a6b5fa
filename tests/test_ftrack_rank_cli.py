"""./pagerank --forward-track FILE --push-eps E --forward-rank K: one `franked` line per set of FILE after the create and after every
batch, `franked <set index> epoch <e> count <found> <v0>:<score0, %.17g> ...`, through dppr_ftrack_topk_ranked -- under
--rank-factor / --rank-exclude when they are given. The lines equal the binding (ForwardTrack.topk_ranked on an engine fed as the
program feeds its own) and numpy (tests/ftrack_rank_ref.py over the track of tests/ftrack_ref.py) batch by batch: the ids and counts
integer for integer, the scores to their 17 digits, which name a double exactly. Without the flag stdout has no such line."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import ftrack_rank_ref as frr
from tests import ftrack_ref as tr
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args
from tests.test_cli import pagerank, run, small_bin  # noqa: F401  (fixtures)
from tests.test_forward_gpu import rows_of

pytestmark = pytest.mark.gpu

EPS, ROUNDS, K = 1e-5, 12, 7


def parse(stdout, n_sets):
    """[[(epoch, ids, scores)] per block]: the create, then every batch."""
    lines = [l.split() for l in stdout.splitlines() if l.startswith("franked ")]
    assert len(lines) == (BATCHES + 1) * n_sets, len(lines)
    out = []
    for b in range(BATCHES + 1):
        block = []
        for i in range(n_sets):
            f = lines[b * n_sets + i]
            assert f[0] == "franked" and int(f[1]) == i and f[2] == "epoch" and f[4] == "count" and len(f) == 6 + int(f[5]), f
            pairs = [x.split(":") for x in f[6:]]
            block.append((int(f[3]), [int(a) for a, _ in pairs], [float(s) for _, s in pairs]))
        out.append(block)
    return out


def reference(V, e1, e2, sets, spec, ref_kw, directed=0):
    """The same stream through the binding and through numpy; the rows of every epoch are read from an engine fed as the program
    feeds its own. Returns the blocks of the binding, after holding them against numpy."""
    g = orc.Graph(V, e1, e2, directed, W, C)
    e = eng.Engine(V, W, directed, C, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    cols = [tr.Column(rows_of(e), ids, w, EPS, ROUNDS) for ids, w in sets]
    seeds = [np.asarray(ids, dtype=np.int64) for ids, _ in sets]
    tracks = [e.ftrack(sets[i:i + 16], EPS, ROUNDS) for i in range(0, len(sets), 16)]

    def block(epoch):
        want = frr.scores([c.p for c in cols], seeds, frr.Graph(V, *e.read_out_graph()), **ref_kw)
        got = [pair for t in tracks for pair in t.topk_ranked(K, 0.0, spec)]
        out = []
        for i, (gi, gs) in enumerate(got):
            wi, ws = frr.topk(want[i], K)
            assert np.array_equal(gi, wi) and np.array_equal(frr.bits(gs), frr.bits(ws)), (epoch, i)
            out.append((epoch, gi.tolist(), gs.tolist()))
        return out

    ref = [block(0)]
    for _ in range(BATCHES):
        assert not g.stream_updates()
        g.inc_construct(1)
        rec = g.batch()
        e.set_batch(*rec)
        epoch = e.slide(*g.new_stream())
        rows = rows_of(e)
        for c in cols:
            c.update(rows, rec, ROUNDS)
        for t in tracks:
            t.update(epoch, ROUNDS)
        ref.append(block(epoch))
    e.close()
    return ref


def test_franked_lines_equal_the_binding_and_numpy(pagerank, small_bin, tmp_path):
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
    rs = eng.Engine.rank_spec
    for extra, spec, ref_kw in (([], None, {}),
                                (["--rank-factor", "deg", "--rank-exclude", "seeds,out"], rs(eng.FACTOR_DEG, exclude=5), dict(factor=frr.DEG, exclude=5)),
                                (["--rank-factor", "inv-deg", "--rank-exclude", "seeds,in,out"], rs(eng.FACTOR_INV_DEG, exclude=7), dict(factor=frr.INV_DEG, exclude=7))):
        r = run(args + flags + ["--forward-rank", str(K)] + extra, env_extra=SERIAL)
        assert r.returncode == 0, r.stdout[-2000:]
        got = parse(r.stdout, len(sets))
        assert got == reference(V, e1, e2, sets, spec, ref_kw), extra
        if not extra:   # a vertex the stream never names is alone in its own raw order; under EXCLUDE_SEEDS the column is empty
            assert got[-1][15][1] == [int(never[0])] and got[-1][15][2] == [0.15]
        else:
            assert got[-1][15][1] == [] and all(sets[i][0][0] not in got[-1][i][1] for i in range(len(sets)))
        assert len(re.findall(r"^ftrack ", r.stdout, re.M)) == len(got) * len(sets)
    beside = run(args + flags + ["--forward-rank", str(K)] + extra)   # the default loop: the next graph is built beside the solve
    assert beside.returncode == 0 and parse(beside.stdout, len(sets)) == got, beside.stdout[-2000:]
    plain = run(args + flags, env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^franked ", plain.stdout, re.M)
