"""./pagerank --certify N: after the initial solve and after every N-th batch, per source in source order, one line
`certify <source> epoch=<id> max_r=<%.17g> at=<v> sum_r=<%.17g> legal=<n_pos + n_neg> nonfinite=<n> inv=<%.17g> inv_at=<v>`, through
dppr_certify / dppr_group_certify with both parts on the epoch the states stand on. Every line has legal=0 nonfinite=0 and inv below
1e-13 * max(1, sum of the lane's seed weights), and the exit code is 0. Without the flag stdout has no such line.

The numbers parse back (%.17g round-trips a double) to what Engine.certify / Engine.group_certify give on the same stream driven
through the Python binding: integers exactly and every double bit for bit -- WHERE a solve repeats itself to the bit. max |r| is a
property of r, and r of a source group on the small .bin does not repeat: the tail of a group's loop pushes with float atomics whose
arrival order differs between two runs (tests/test_cli.py holds two such runs to 1e-14, not to the bit). Measured here, the same
stream solved twice from scratch by a 3-source group under --sync: max_r = 9.83082660019702e-10 in one run and
9.830826600197021e-10 in the other, and the invariant's rounding-level maximum (2.1e-17 against 2.8e-17) at another vertex. So:
  * on the stream of one out-edge per vertex (tests/test_changes_cli.py: every residual receives at most one add per iteration, so
    the solve is the same to the bit whatever the order of arrival) a source GROUP and a single source are both held to the binding
    value for value, every double to the bit, in ./pagerank's serial loop; the single source in the default, overlapped loop too;
  * on the small .bin a group's lines are held bit for bit (max_r, sum_r; at, legal, nonfinite exactly; inv to 1e-13) to the numpy
    restatement (tests/certify_ref.py) over the state ./pagerank itself dumps after the last batch, and to the binding's second
    solve at the project's bound for two solves, 1e-14."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import certify_ref as cr
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args, one_out_stream
from tests.test_cli import pagerank, read_dump, run, small_bin  # noqa: F401  (fixtures)
from tests.util import window_directed_edges

pytestmark = pytest.mark.gpu

EPS = 1e-9
TWO_SOLVES = 1e-14   # tests/test_cli.py: two runs of one stream under the synchronous schedule
LINE = re.compile(r"^certify (\d+) epoch=(-?\d+) max_r=(\S+) at=(-?\d+) sum_r=(\S+) legal=(\d+) nonfinite=(\d+) inv=(\S+) inv_at=(-?\d+)$")


def parse(stdout, sources, blocks):
    """[{source: (epoch, max_r, at, sum_r, legal, nonfinite, inv, inv_at)} per block]; asserts the form and the order of the lines."""
    lines = [l for l in stdout.splitlines() if l.startswith("certify ")]
    assert len(lines) == blocks * len(sources), (len(lines), blocks, stdout[-1500:])
    out = []
    for b in range(blocks):
        block = {}
        for j, s in enumerate(sources):
            m = LINE.match(lines[b * len(sources) + j])
            assert m and int(m.group(1)) == s, lines[b * len(sources) + j]
            block[s] = (int(m.group(2)), float(m.group(3)), int(m.group(4)), float(m.group(5)), int(m.group(6)), int(m.group(7)),
                        float(m.group(8)), int(m.group(9)))
        out.append(block)
    return out


def feed(V, e1, e2, sources, as_group, directed, every=1):
    """The same stream through the binding: one certificate after the from-scratch solve and one after every `every`-th batch.
    Returns the blocks in the form of parse() and the oracle graph at the last batch."""
    g = orc.Graph(V, e1, e2, directed, W, C)
    e = eng.Engine(V, W, directed, C, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    h = e.add_source_group(sources) if as_group else e.add_source(sources[0])
    (e.group_init_solve if as_group else e.init_solve)(h, EPS)
    out = []

    def certificate():
        res = (e.group_certify if as_group else e.certify)(h, EPS)
        out.append({s: (res["state_epoch"], float(res["max_abs_r"][i]), int(res["argmax_r"][i]), float(res["sum_abs_r"][i]),
                        int(res["n_pos"][i] + res["n_neg"][i]), int(res["n_nonfinite"][i]), float(res["inv_max_err"][i]),
                        int(res["inv_argmax"][i])) for i, s in enumerate(sources)})

    certificate()
    for b in range(1, BATCHES + 1):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        (e.group_update if as_group else e.update)(h, EPS)
        if b % every == 0:
            certificate()
    e.close()
    return out, g


def healthy(blocks, every=1):
    for blk in blocks:
        for epoch, max_r, at, sum_r, legal, nonfinite, inv, inv_at in blk.values():
            assert legal == 0 and nonfinite == 0 and 0.0 <= max_r < EPS and max_r <= sum_r and at >= 0, blk
            assert 0.0 <= inv < 1e-13 and inv_at >= 0, blk
    for s in blocks[0]:
        assert [blk[s][0] for blk in blocks] == list(range(0, BATCHES + 1, every))   # the epoch the state stands on


@pytest.mark.parametrize("every", [1, 2])
def test_sources_file_as_a_group(pagerank, small_bin, tmp_path, every):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, 3)]
    sf = tmp_path / "sources.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    dump = str(tmp_path / "dump.bin")
    r = run([pagerank] + base_args(path) + ["--sources", str(sf), "--certify", str(every), "--dump", dump], env_extra=SERIAL)
    assert r.returncode == 0 and "CERTIFY FAILED" not in r.stdout, r.stdout[-2000:]
    got = parse(r.stdout, sources, 1 + BATCHES // every)
    healthy(got, every)
    # the last block against numpy over the state ./pagerank dumped itself: the line is the certificate of that very state
    want, g = feed(V, e1, e2, sources, True, 0, every)
    state = read_dump(dump)
    tails, heads = window_directed_edges(g)
    ref = cr.certify(V, tails, heads, [state[s][0] for s in sources], [state[s][1] for s in sources], sources, EPS)
    for i, s in enumerate(sources):
        epoch, max_r, at, sum_r, legal, nonfinite, inv, inv_at = got[-1][s]
        assert (max_r, at, sum_r) == (ref["max_abs_r"][i], ref["argmax_r"][i], ref["sum_abs_r"][i]), (s, got[-1][s], ref)   # bit for bit
        assert legal == ref["n_pos"][i] + ref["n_neg"][i] and nonfinite == ref["n_nonfinite"][i]
        assert abs(inv - ref["inv_max_err"][i]) < 1e-13 and abs(ref["err"][i][inv_at] - inv) < 1e-13
    # ... and against the binding's own solve of the same stream, as far as two solves of a group agree
    assert len(want) == len(got)
    for a, b in zip(got, want):
        for s in sources:
            assert a[s][0] == b[s][0] and a[s][4:6] == b[s][4:6], (a[s], b[s])                        # epoch, legal, nonfinite
            assert abs(a[s][1] - b[s][1]) < TWO_SOLVES and abs(a[s][3] - b[s][3]) < V * TWO_SOLVES and abs(a[s][6] - b[s][6]) < 1e-13, (a[s], b[s])
    if every == 1:
        plain = run([pagerank] + base_args(path) + ["--sources", str(sf)], env_extra=SERIAL)
        assert plain.returncode == 0 and not re.search(r"^certify ", plain.stdout, re.M)
        beside = run([pagerank] + base_args(path) + ["--sources", str(sf), "--certify", "1"])   # the default loop: the explicit epoch
        assert beside.returncode == 0 and "CERTIFY FAILED" not in beside.stdout, beside.stdout[-2000:]
        healthy(parse(beside.stdout, sources, 1 + BATCHES))


@pytest.mark.parametrize("sources", [[0], [0, 1, 2]], ids=["slot", "group"])
def test_one_out_stream_bit_for_bit(pagerank, tmp_path, sources):
    V, e1, e2 = one_out_stream()
    for lo in range(0, BATCHES * C + 1, C):  # the property the comparison rests on: one out-edge per vertex in window + batch
        assert len(np.unique(e1[lo:lo + W + C])) == W + C
    path = str(tmp_path / "one_out.bin")
    datagen.write_bin(path, V, e1, e2)
    as_group = len(sources) > 1
    if as_group:
        sf = tmp_path / "sources.txt"
        sf.write_text("\n".join(map(str, sources)) + "\n")
        args = [pagerank] + base_args(path, directed=1) + ["--sources", str(sf), "--certify", "1"]
    else:
        args = [pagerank] + base_args(path, directed=1) + ["-s", "0", "--certify", "1"]
    r = run(args, env_extra=SERIAL)
    assert r.returncode == 0 and "CERTIFY FAILED" not in r.stdout, r.stdout[-2000:]
    got = parse(r.stdout, sources, 1 + BATCHES)
    healthy(got)
    want, _ = feed(V, e1, e2, sources, as_group, 1)
    assert got == want, (got, want)   # integers exactly, max_r, sum_r and inv bit for bit through %.17g
    beside = run(args)  # the default loop: the next graph is built beside the solve, the certificate names its epoch
    assert beside.returncode == 0 and "CERTIFY FAILED" not in beside.stdout, beside.stdout[-2000:]
    other = parse(beside.stdout, sources, 1 + BATCHES)
    healthy(other)
    if not as_group:   # (a group's solve in the overlapped loop is not among the premises: tests/test_explain_cli.py)
        assert other == got
