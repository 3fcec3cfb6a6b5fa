"""./pagerank --sample S [--sample-seed X] [--rank-factor F] [--rank-exclude X]: after every batch, per source in source order, one
line `sample <source> lane <lane> total <t> support <n> status <s> distinct <d> ids <the first 8>`, through dppr_sample /
dppr_group_sample on the epoch the states stand on. The lines equal what Engine.sample / Engine.group_sample give on the same
stream driven through the Python binding -- the ids integer for integer, the total to its 17 digits --, batch by batch.
That comparison of two solves needs streams on which a solve repeats itself to the bit, the ones tests/test_changes_cli.py rests
on: a source GROUP on the small .bin under the synchronous schedule (its sweeps gather), and for a single source the stream of one
out-edge per vertex. ./pagerank runs its serial batch loop (the binding's call sequence) and, once, the default overlapped one.
Without the flag stdout has no such line."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args, one_out_stream
from tests.test_cli import pagerank, run, small_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

DRAWS = 64


def parse(stdout, sources):
    """[{source: (lane, total, support, status, distinct, [first 8 ids])} per batch]; asserts the order of the lines."""
    lines = [l.split() for l in stdout.splitlines() if l.startswith("sample ")]
    assert len(lines) == BATCHES * len(sources), len(lines)
    out = []
    for b in range(BATCHES):
        block = {}
        for i, s in enumerate(sources):
            f = lines[b * len(sources) + i]
            assert [f[0], f[2], f[4], f[6], f[8], f[10], f[12]] == ["sample", "lane", "total", "support", "status", "distinct", "ids"] and int(f[1]) == s, f
            block[s] = (int(f[3]), float(f[5]), int(f[7]), int(f[9]), int(f[11]), [int(x) for x in f[13:]])
        out.append(block)
    return out


def feed(V, e1, e2, sources, as_group, spec, directed, seed):
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
            ids, _, total, support, status = e.group_sample(h, DRAWS, spec, 0.0, seed, 0, with_w=False)
        else:
            e.update(h, 1e-9)
            ids, _, total, support, status = e.sample(h, DRAWS, spec, 0.0, seed, 0, with_w=False)
            ids, total, support, status = ids[None, :], [total], [support], [status]
        out.append({s: (i, float(total[i]), int(support[i]), int(status[i]), len(np.unique(ids[i][ids[i] >= 0])), ids[i][:8].tolist())
                    for i, s in enumerate(sources)})
    e.close()
    return out


@pytest.mark.parametrize("rank,spec,seed", [([], None, 0), (["--rank-factor", "deg", "--rank-exclude", "seeds,in"], (eng.FACTOR_DEG, 3), 12345)])
def test_sources_file_as_a_group(pagerank, small_bin, tmp_path, rank, spec, seed):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, 3)]
    sf = tmp_path / "sources.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    args = [pagerank] + base_args(path) + ["--sources", str(sf), "--sample", str(DRAWS)] + (["--sample-seed", str(seed)] if seed else []) + rank
    r = run(args, env_extra=SERIAL)
    assert r.returncode == 0, r.stdout
    got = parse(r.stdout, sources)
    sp = eng.Engine.rank_spec(spec[0], exclude=spec[1]) if spec else None
    assert got == feed(V, e1, e2, sources, True, sp, 0, seed)
    last = got[-1]
    assert all(last[s][3] == eng.SAMPLE_OK and 1 <= last[s][4] <= DRAWS and len(last[s][5]) == 8 and last[s][0] == i for i, s in enumerate(sources))
    if spec and spec[1] & 1:
        assert all(s not in last[s][5] for s in sources)          # the seed itself is out of its own lane
    if not rank:
        beside = run(args)  # the default loop: the next graph is built beside the solve
        assert beside.returncode == 0 and parse(beside.stdout, sources) == got, beside.stdout[-2000:]
        plain = run([pagerank] + base_args(path) + ["--sources", str(sf)], env_extra=SERIAL)
        assert plain.returncode == 0 and not re.search(r"^sample ", plain.stdout, re.M)


def test_one_source(pagerank, tmp_path):
    V, e1, e2 = one_out_stream()
    path = str(tmp_path / "one_out.bin")
    datagen.write_bin(path, V, e1, e2)
    r = run([pagerank] + base_args(path, directed=1) + ["-s", "0", "--sample", str(DRAWS), "--sample-seed", "0x10", "--rank-factor", "inv-deg"], env_extra=SERIAL)
    assert r.returncode == 0, r.stdout
    got = parse(r.stdout, [0])
    assert got == feed(V, e1, e2, [0], False, eng.Engine.rank_spec(eng.FACTOR_INV_DEG), 1, 16)
    assert all(blk[0][3] == eng.SAMPLE_OK for blk in got)
