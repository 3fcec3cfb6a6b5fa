"""./pagerank --refine FILE --walks W [--walk-seed S]: after every batch one line `refined <vertex> <source index> <est> <corr>
<stderr>` per listed vertex and per source, through dppr_refine_at / dppr_group_refine_at. The lines of the last batch equal, bit
for bit (%.17g round-trips a double), the formula of include/dppr.h over --dump and the endpoints dppr_walks returns for the same
stream driven through the binding; the lines of every batch agree with dppr_group_refine_at of the binding (two solves of one
stream agree to far below the tolerance, not always to the bit: the correction is compared to 1e-12). Without the flag stdout has
no such line and is otherwise the same sequence of lines."""
import re

import numpy as np
import pytest

from dynamicppr_amd import datagen, engine as eng
from oracle import oracle as orc
from tests import dot_ref, walk_ref
from tests.test_changes_cli import BATCHES, C, SERIAL, W, base_args
from tests.test_cli import pagerank, read_dump, run, small_bin  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

WALKS, SEED = 300, (7 << 32) | 11


def parse(stdout, ids, n_src):
    """[batch][vertex position][source index] -> (est, corr, stderr); asserts the order of the lines."""
    lines = [l.split() for l in stdout.splitlines() if l.startswith("refined ")]
    assert len(lines) == BATCHES * len(ids) * n_src and all(len(l) == 6 for l in lines)
    want_keys = [(v, j) for _ in range(BATCHES) for v in ids for j in range(n_src)]
    assert [(int(l[1]), int(l[2])) for l in lines] == want_keys  # batch by batch, by vertex, then source order
    return np.array([[float(x) for x in l[3:]] for l in lines]).reshape(BATCHES, len(ids), n_src, 3)


def binding(V, e1, e2, sources, ids):
    """The same stream through the binding: per batch the endpoints (dppr_walks) and dppr_group_refine_at."""
    g = orc.Graph(V, e1, e2, 0, W, C)
    e = eng.Engine(V, W, 0, C, schedule=eng.SCHEDULE_SYNC)
    e.load_window(*g.window_edges())
    gid = e.add_source_group(sources)
    e.group_init_solve(gid, 1e-9)
    out = []
    for _ in range(BATCHES):
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        e.group_update(gid, 1e-9)
        out.append((e.walks(ids, WALKS, SEED),) + e.group_refine_at(gid, ids, WALKS, SEED))
    e.close()
    return out


@pytest.mark.parametrize("n_src", [1, 3])
def test_refined_lines_equal_the_abi_call(pagerank, small_bin, tmp_path, n_src):
    path, V, e1, e2 = small_bin
    sources = [int(x) for x in datagen.top_sources(V, e1, e2, W, 0, n_src)]
    named = np.zeros(V, dtype=bool)
    named[e1] = named[e2] = True
    ids = [sources[0], int(np.nonzero(~named)[0][0]) if not named.all() else 0, int(e1[5]), sources[0]]
    rf, srcf, dump = tmp_path / "refine.txt", tmp_path / "sources.txt", str(tmp_path / "out.dump")
    rf.write_text("\n".join(map(str, ids)) + "\n")
    srcf.write_text("\n".join(map(str, sources)) + "\n")
    args = [pagerank] + base_args(path) + (["-s", str(sources[0])] if n_src == 1 else ["--sources", str(srcf)])
    flags = ["--refine", str(rf), "--walks", str(WALKS), "--walk-seed", str(SEED)]
    r = run(args + ["--dump", dump] + flags, env_extra=SERIAL)
    assert r.returncode == 0, r.stdout
    got = parse(r.stdout, ids, n_src)
    ref = binding(V, e1, e2, sources, np.array(ids, dtype=np.int32))
    dumps = read_dump(dump)
    # the last batch: the stated formula over the dumped state and the endpoints, to the bit
    ends = ref[-1][0]
    ps, rs = [dumps[s][0] for s in sources], [dumps[s][1] for s in sources]
    t = walk_ref.terms(ends, rs)
    corr = (dot_ref.fold(t) / float(WALKS)).T
    est = (np.stack(ps)[:, ids] + corr.T).T
    sumsq = dot_ref.fold(t * t).T
    se = np.sqrt(np.maximum(sumsq / WALKS - corr * corr, 0.0) / (WALKS - 1.0))
    for k, want in enumerate((est, corr)):
        assert np.array_equal(got[-1, :, :, k].view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (k, got[-1, :, :, k], want)
    assert np.allclose(got[-1, :, :, 2], se, rtol=1e-9, atol=0.0)  # (derived on the host from sumsq: the formula of INTEGRATION.md)
    assert np.any(corr != 0.0)
    # every batch: the binding's call
    for b in range(BATCHES):
        _, b_est, b_corr, _ = ref[b]
        assert np.max(np.abs(got[b, :, :, 0] - b_est)) < 1e-12 and np.max(np.abs(got[b, :, :, 1] - b_corr)) < 1e-12, b
    # the default, overlapped loop prints the same lines (the state stands on the epoch it names, not on the newest)
    o = run(args + flags)
    assert o.returncode == 0, o.stdout
    assert np.max(np.abs(parse(o.stdout, ids, n_src)[..., :2] - got[..., :2])) < 1e-12
    # without the flag: no such line, and otherwise the same sequence of lines
    plain = run(args + ["--dump", str(tmp_path / "plain.dump")], env_extra=SERIAL)
    assert plain.returncode == 0 and not re.search(r"^refined ", plain.stdout, re.M)

    def shape(text):  # (what every line begins with; the child's two streams share one pipe, so the order is not compared)
        return sorted(l.split()[0].split("=")[0] for l in text.splitlines() if l.strip() and not l.startswith("refined "))

    assert shape(r.stdout) == shape(plain.stdout)


def test_bad_arguments_are_rejected(pagerank, small_bin, tmp_path):
    path, V, _, _ = small_bin
    good, empty, beyond, negative = (tmp_path / n for n in ("good.txt", "empty.txt", "beyond.txt", "negative.txt"))
    good.write_text("0\n1\n")
    empty.write_text("")
    beyond.write_text(f"0\n{V}\n")
    negative.write_text("0\n-1\n")
    cases = [["--refine", str(good)], ["--walks", "10"], ["--refine", str(good), "--walks", "0"],
             ["--refine", str(good), "--walks", str((1 << 20) + 1)]]
    cases += [["--refine", bad, "--walks", "10"] for bad in (str(tmp_path / "missing.txt"), str(empty), str(beyond), str(negative))]
    for extra in cases:
        r = run([pagerank] + base_args(path) + extra)
        assert r.returncode != 0 and "invalid arguments" in r.stdout and not re.search(r"^refined ", r.stdout, re.M), extra
