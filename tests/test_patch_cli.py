"""./pagerank --patch-min P [--patch-delta D] [--patch-out FILE]: the from-scratch solution is the mark; after every batch one line
`patch <source> upserts <a> deletes <b>` per source in source order, through dppr_patch / dppr_group_patch with the emitted-only
re-mark, and in FILE one line `U <batch> <source> <vertex> <pagerank>` per upsert and `D <batch> <source> <vertex>` per delete, by
source then vertex id. The lines and the file equal tests/patch_ref.py over the dense reads of the same stream driven through the
Python binding, the reference's mark re-marked as the program re-marks; %.17g round-trips a double.

Two solves of one stream can only be compared bit for bit where the solver itself is reproducible (tests/test_changes_cli.py has
the argument). Neither the single-source solver nor a source group is on the small .bin: pushes that reach one residual in the
same iteration add in arrival order, and a group's p there was seen to differ in the last place between ./pagerank and the
binding (0.006895327455330586 against ...587), in the serial loop as in the overlapped one. So the bit comparison runs on
one_out_stream of tests/test_changes_cli.py -- every vertex has at most one out-edge in any window plus batch, so every residual of
every lane receives at most one add per iteration -- for a slot and for a five-source group, on the synchronous schedule with
./pagerank's serial batch loop (DPPR_NO_OVERLAP=1: the binding's call sequence); the slot's default, overlapped loop is held to the
same bits, the group's to the structure. The group on the small .bin is held to the structure alone: the lines in order, the
file's entries per batch and source as many as the lines say, every kind by ascending id, every upsert above P. Without the flag
stdout is what it was."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import patch_ref as ref
from tests.test_changes_cli import SERIAL, C, W, one_out_stream
from tests.test_cli import pagerank, run, small_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BATCHES = 3
MIN_P, DELTA = 1e-3, 1e-7


def base_args(path, directed=0):
    return ["-d", path, "-a", "0", "-i", str(directed), "-y", "1", "-n", "0", "-r", "0.01", "-b", str(BATCHES), "--sync"]


def feed(V, e1, e2, sources, delta, as_group, directed):
    """The same stream through the binding: the dense reads after the from-scratch solve and after every batch, the reference's patch
    against the reference's mark, re-marked at the emitted entries. [(the patch of batch 1), ..]"""
    g = orc.Graph(V, e1, e2, directed, W, C)
    e = eng.Engine(V, W, directed, C, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    h = e.add_source_group(sources) if as_group else e.add_source(sources[0])
    if as_group:
        e.group_init_solve(h, 1e-9)
    else:
        e.init_solve(h, 1e-9)
    dense = lambda: [e.group_read(h, i)[0] for i in range(len(sources))] if as_group else [e.read(h)[0]]
    mark = dense()
    out = []
    for _ in range(BATCHES):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        if as_group:
            e.group_update(h, 1e-9)
        else:
            e.update(h, 1e-9)
        now = dense()
        out.append(ref.patch(now, mark, MIN_P, delta))
        mark = ref.remark(now, mark, MIN_P, delta, ref.REMARK_EMITTED)
    e.close()
    return out


def parse(stdout, text, sources):
    lines = [l.split() for l in stdout.splitlines() if l.startswith("patch ")]
    assert all(len(l) == 6 and l[2] == "upserts" and l[4] == "deletes" for l in lines)
    assert [int(l[1]) for l in lines] == sources * BATCHES  # batch by batch, in source order
    return lines, [l.split() for l in text.splitlines()]


def check_structure(stdout, text, sources):
    lines, rows = parse(stdout, text, sources)
    at = 0
    for b in range(BATCHES):
        for j, s in enumerate(sources):
            for kind, count, width in (("U", int(lines[b * len(sources) + j][3]), 5), ("D", int(lines[b * len(sources) + j][5]), 4)):
                mine = rows[at:at + count]
                at += count
                assert len(mine) == count and all(len(r) == width and r[:3] == [kind, str(b + 1), str(s)] for r in mine), (b, s, kind)
                ids = [int(r[3]) for r in mine]
                assert ids == sorted(set(ids)), (b, s, kind)
                assert kind == "D" or all(float(r[4]) > MIN_P for r in mine), (b, s)
    assert at == len(rows)


def check(stdout, text, want, sources):
    lines, rows = parse(stdout, text, sources)
    at = 0
    for b, pt in enumerate(want):
        for j, s in enumerate(sources):
            line = lines[b * len(sources) + j]
            uo, do = pt["up_offsets"], pt["del_offsets"]
            assert (int(line[3]), int(line[5])) == (uo[j + 1] - uo[j], do[j + 1] - do[j]), (b, s, line)
            for t in range(uo[j], uo[j + 1]):
                assert rows[at][:4] == ["U", str(b + 1), str(s), str(pt["up_ids"][t])] and float(rows[at][4]) == pt["up_p"][t], (b, s, rows[at])
                at += 1
            for t in range(do[j], do[j + 1]):
                assert rows[at] == ["D", str(b + 1), str(s), str(pt["del_ids"][t])], (b, s, rows[at])
                at += 1
    assert at == len(rows)


def patch_flags(out, delta):
    return ["--patch-min", str(MIN_P), "--patch-out", str(out)] + (["--patch-delta", str(delta)] if delta is not None else [])


@pytest.mark.parametrize("delta", [None, DELTA])
@pytest.mark.parametrize("as_group", [False, True])
def test_one_out_stream_bit_for_bit(pagerank, tmp_path, as_group, delta):
    V, e1, e2 = one_out_stream()
    for lo in range(0, BATCHES * C + 1, C):  # the property the bit comparison rests on: one out-edge per vertex in window + batch
        assert len(np.unique(e1[lo:lo + W + C])) == W + C
    path = str(tmp_path / "one_out.bin")
    datagen.write_bin(path, V, e1, e2)
    sources = [0, 1, 2, 3, 4] if as_group else [0]
    if as_group:
        sf = tmp_path / "sources.txt"
        sf.write_text("\n".join(map(str, sources)) + "\n")
        who = ["--sources", str(sf)]
    else:
        who = ["-s", "0"]
    out = tmp_path / "patch.txt"
    out.write_text("stale\n")  # (the file starts empty whatever it held)
    args = base_args(path, directed=1) + who
    r = run([pagerank] + args + patch_flags(out, delta), env_extra=SERIAL)
    assert r.returncode == 0, r.stdout
    want = feed(V, e1, e2, sources, delta or 0.0, as_group, 1)
    assert all(pt["up_offsets"][-1] > 0 and pt["del_offsets"][-1] > 0 for pt in want)  # the reference shows both kinds in every batch
    check(r.stdout, out.read_text(), want, sources)
    check_structure(r.stdout, out.read_text(), sources)
    beside = run([pagerank] + args + patch_flags(out, delta))  # the default loop: the next graph is built beside the solve
    assert beside.returncode == 0, beside.stdout
    if as_group:
        check_structure(beside.stdout, out.read_text(), sources)
    else:
        check(beside.stdout, out.read_text(), want, sources)
    plain = run([pagerank] + args, env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^patch ", plain.stdout, re.M)
    # what the timed region reports does not depend on the flag: the same lines, in the same number
    keys = r"^(coming stream_batch_count=\d+|edge_num \d+)$"
    assert re.findall(keys, r.stdout, re.M) == re.findall(keys, plain.stdout, re.M)
    assert len([l for l in r.stdout.splitlines() if not l.startswith("patch ")]) == len(plain.stdout.splitlines())


@pytest.mark.parametrize("delta", [None, DELTA])
def test_sources_file_as_a_group(pagerank, small_bin, tmp_path, delta):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, 5)]
    sf = tmp_path / "sources.txt"
    sf.write_text("\n".join(map(str, sources)) + "\n")
    out = tmp_path / "patch.txt"
    for env in (SERIAL, None):
        r = run([pagerank] + base_args(path) + ["--sources", str(sf)] + patch_flags(out, delta), env_extra=env)
        assert r.returncode == 0, r.stdout
        check_structure(r.stdout, out.read_text(), sources)
        lines, rows = parse(r.stdout, out.read_text(), sources)
        assert sum(int(l[3]) for l in lines) > 0 and sum(int(l[5]) for l in lines) > 0  # both kinds were fed
    plain = run([pagerank] + base_args(path) + ["--sources", str(sf)], env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^patch ", plain.stdout, re.M)
    assert len([l for l in r.stdout.splitlines() if not l.startswith("patch ")]) == len(plain.stdout.splitlines())
