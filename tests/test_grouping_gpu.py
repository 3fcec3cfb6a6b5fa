"""The grouping of a batch's records by tail (IncrementalBatchUpdate's first step), read back through dppr_debug_grouping and
compared with numpy on every path, at the path and tile boundaries, for the tail distributions that stress each path.

Contract (dynamicppr_amd/csrc/dppr_grouping.hpp): equal tails are contiguous and keep batch order. Rank, radix and the at-slide
arrays give tails ascending, i.e. exactly np.argsort(tails, kind="stable"); bucket gives bucket (tail & (nb - 1)) order, tails
ascending inside a bucket, batch order inside a tail, i.e. exactly np.lexsort((i, t, t & (nb - 1))).

One engine serves the module: its window holds every vertex (so internal ids never change), and every batch is uploaded by a
slide that adds no edge. The batches are built in INTERNAL ids (the ones the kernels see) through the map a probe batch reveals."""
import numpy as np
import pytest

from dynamicppr_amd import engine as eng

pytestmark = pytest.mark.gpu

RANK, BUCKET, RADIX, AT_SLIDE = 1, 2, 3, 4
SU_RANK_MAX, SU_GRP_MAX_RECORDS, SU_GRP_MAX_BUCKET = 4096, 1 << 22, 1 << 14
V = 1 << 21
C_MAX = (1 << 20) + 1           # 4 * C_MAX records >= 4 Mi + 1
MI = 1 << 20


def buckets(L):
    nb = 64
    while nb < 4096 and nb * 512 < L:
        nb *= 2
    return nb


def expected_auto_path(t):
    """dppr_grouping.hpp grouping_path, restated."""
    L = len(t)
    if L <= SU_RANK_MAX:
        return RANK
    if L <= SU_GRP_MAX_RECORDS and np.bincount(t & (buckets(L) - 1)).max() <= SU_GRP_MAX_BUCKET:
        return BUCKET
    return RADIX


class Rig:
    def __init__(self):
        rng = np.random.default_rng(1)
        # every vertex is a tail and a head of the window: all of them have internal ids from load_window on
        w1 = rng.permutation(V).astype(np.int32)
        w2 = np.roll(w1, 1)
        self.e = eng.Engine(V, V, 1, C_MAX)
        self.e.set_renumbering(0)
        self.e.load_window(w1, w2)
        self.e.set_batch_grouping(1)
        # probe batch: record i has external tail i, so its raw (internal) tail is the map
        self.upload(np.arange(V, dtype=np.int32))
        _, _, raw, _, _ = self.e.debug_grouping(path=RADIX)
        self.ext2int = raw.astype(np.int64)
        assert np.array_equal(np.sort(self.ext2int), np.arange(V))
        self.int2ext = np.empty(V, np.int32)
        self.int2ext[self.ext2int] = np.arange(V, dtype=np.int32)

    def upload(self, ext_tails, at_slide=1):
        L = len(ext_tails)
        rng = np.random.default_rng(L)
        heads = rng.integers(0, V, L).astype(np.int32)
        ins = (rng.random(L) < 0.5).astype(np.uint8)
        self.e.set_batch_grouping(at_slide)
        self.e.set_batch(ext_tails, heads, ins)
        return self.e.slide(np.zeros(0, np.int32), np.zeros(0, np.int32))

    def upload_internal(self, t, at_slide=1):
        ep = self.upload(self.int2ext[t], at_slide)
        return ep


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.e.close()


def tails_for(dist, L, rng):
    """Internal tails of an L-record batch."""
    if dist == "uniform":
        return rng.integers(0, V, L)
    if dist == "one-tail":
        return np.full(L, 12345)
    if dist == "id-space-edges":
        return np.where(rng.random(L) < 0.5, 0, V - 1)
    if dist == "two-hubs-one-bucket":          # t and t + nb share the low bits: one bucket, two tails
        t0 = 77
        return np.where(rng.random(L) < 0.5, t0, t0 + buckets(L))
    if dist == "distinct-descending":          # all distinct while L <= V, then descending runs
        i = np.arange(L, dtype=np.int64)
        return (V - 1) - (i if L <= V else i * V // L)
    if dist == "hub-across-chunks":            # every 2 048-record chunk of k_su_grp_hist / _scatter holds a slice of the hub
        t = rng.integers(0, V, L)
        t[(np.arange(L) % 2048) % 3 == 0] = 4242
        return t
    if dist == "hub-90pct":
        return np.where(rng.random(L) < 0.9, 999, rng.integers(0, V, L))
    raise ValueError(dist)


def check_contract(t, gt, gi):
    """Every path: a permutation, every tail one contiguous run, indices increasing inside a run."""
    L = len(t)
    assert len(gt) == L and len(gi) == L
    assert np.array_equal(np.sort(gi.astype(np.int64)), np.arange(L)), "not a permutation of the records"
    assert np.array_equal(gt.astype(np.int64), t[gi.astype(np.int64)]), "tail does not belong to its record"
    if L > 1:
        starts = np.flatnonzero(np.diff(gt.astype(np.int64)) != 0) + 1
        run_tails = gt[np.concatenate([[0], starts])]
        assert len(np.unique(run_tails)) == len(run_tails), "a tail is split into several runs"
        same = np.diff(gt.astype(np.int64)) == 0
        assert np.all(np.diff(gi.astype(np.int64))[same] > 0), "batch order broken inside a tail"


class Want:
    """The reference orders of one batch, computed once."""

    def __init__(self, t):
        self.t = t
        self._w = {}

    def __call__(self, bucketed):
        if bucketed not in self._w:
            t = self.t
            self._w[bucketed] = (np.lexsort((np.arange(len(t)), t, t & (buckets(len(t)) - 1))) if bucketed
                                 else np.argsort(t, kind="stable"))
        return self._w[bucketed]


def check_path(rig, want, path):
    t = want.t
    gt, gi, raw, taken, nb = rig.e.debug_grouping(path=path)
    assert np.array_equal(raw.astype(np.int64), t), "the epoch's raw tails are not the uploaded ones"
    check_contract(t, gt, gi)
    if taken == BUCKET:
        assert nb == buckets(len(t))
    else:
        assert nb == 0
    want = want(taken == BUCKET)
    assert np.array_equal(gi.astype(np.int64), want), f"path {taken}: record order differs from the reference"
    assert np.array_equal(gt.astype(np.int64), t[want]), f"path {taken}: tails differ from the reference"
    return taken


def run_all_paths(rig, t):
    L = len(t)
    want = Want(np.asarray(t, np.int64))
    rig.upload_internal(t, at_slide=1)
    assert check_path(rig, want, 0) == AT_SLIDE        # an epoch grouped at slide: the timed region reads those arrays
    assert check_path(rig, want, AT_SLIDE) == AT_SLIDE
    if L <= 65536:
        assert check_path(rig, want, RANK) == RANK
    if L <= SU_GRP_MAX_RECORDS:
        assert check_path(rig, want, BUCKET) == BUCKET
    assert check_path(rig, want, RADIX) == RADIX
    # the same batch grouped inside the timed region: the path its length and fullest bucket select
    rig.upload_internal(t, at_slide=0)
    assert check_path(rig, want, 0) == expected_auto_path(t)


SMALL = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097]
# every step of nb (64 -> 128 at 32 769 records ... 2 048 -> 4 096 at 2 Mi + 1)
STEPS = [n + d for n in (32768, 65536, 131072, 262144, 524288, 1 << 20, 1 << 21) for d in (0, 1)]
DISTS = ["uniform", "one-tail", "id-space-edges", "two-hubs-one-bucket", "distinct-descending", "hub-across-chunks", "hub-90pct"]


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("L", SMALL + STEPS)
def test_grouping_every_path_equals_numpy(rig, L, dist):
    run_all_paths(rig, tails_for(dist, L, np.random.default_rng(L * 7 + len(dist))))


@pytest.mark.parametrize("dist", ["uniform", "one-tail"])
@pytest.mark.parametrize("L", [4 * MI - 1, 4 * MI, 4 * MI + 1])
def test_grouping_at_the_radix_boundary(rig, L, dist):
    """4 Mi records is the last length of the bucket path: one more and the radix sort is selected by length alone."""
    t = tails_for(dist, L, np.random.default_rng(L))
    run_all_paths(rig, t)
    if dist == "uniform":
        assert expected_auto_path(t) == (BUCKET if L <= SU_GRP_MAX_RECORDS else RADIX)


def test_hot_bucket_goes_to_radix_and_uniform_stays_on_bucket(rig):
    """A bucket of more than SU_GRP_MAX_BUCKET records sends the batch to the radix sort; one record fewer keeps it on buckets."""
    rng = np.random.default_rng(5)
    L = MI
    nb = buckets(L)
    for hot, path in ((SU_GRP_MAX_BUCKET, BUCKET), (SU_GRP_MAX_BUCKET + 1, RADIX)):
        t = rng.integers(0, V, L)
        t = np.where((t & (nb - 1)) == 0, t + 1, t)       # bucket 0 holds exactly the hot records (tail 0)
        t[rng.choice(L, hot, replace=False)] = 0
        assert np.bincount(t & (nb - 1)).max() == hot
        rig.upload_internal(t, at_slide=0)
        assert check_path(rig, Want(t), 0) == path


@pytest.mark.parametrize("path", [-1, 5])
def test_debug_grouping_rejects_bad_arguments(rig, path):
    rig.upload_internal(np.arange(5000), at_slide=0)
    with pytest.raises(eng.DpprError):
        rig.e.debug_grouping(path=path)
    with pytest.raises(eng.DpprError):
        rig.e.debug_grouping(path=AT_SLIDE)            # not grouped at slide
    with pytest.raises(eng.DpprError):
        rig.e.debug_grouping(epoch=10 ** 6, path=RADIX)  # not resident
    rig.upload_internal(np.zeros(65537, np.int64), at_slide=0)
    with pytest.raises(eng.DpprError):
        rig.e.debug_grouping(path=RANK)                # quadratic: at most 64 Ki records
    rig.upload_internal(np.arange(SU_GRP_MAX_RECORDS + 1) % V, at_slide=0)
    with pytest.raises(eng.DpprError):
        rig.e.debug_grouping(path=BUCKET)              # beyond 4 Mi records


def test_grouping_radix_switch_selects_radix(monkeypatch):
    """DPPR_GROUPING_RADIX=1: path 0 reports the radix sort for a batch that would otherwise be bucketed or ranked."""
    monkeypatch.setenv("DPPR_GROUPING_RADIX", "1")
    n = 1 << 16
    rng = np.random.default_rng(9)
    w1 = rng.permutation(n).astype(np.int32)
    e = eng.Engine(n, n, 1, 1 << 14)
    try:
        e.load_window(w1, np.roll(w1, 1))
        for L in (100, 50000):
            b1 = rng.integers(0, n, L).astype(np.int32)
            e.set_batch(b1, rng.integers(0, n, L).astype(np.int32), np.ones(L, np.uint8))
            e.slide(np.zeros(0, np.int32), np.zeros(0, np.int32))
            gt, gi, raw, taken, nb = e.debug_grouping(path=0)
            assert taken == RADIX and nb == 0
            want = np.argsort(raw, kind="stable")
            assert np.array_equal(gi.astype(np.int64), want)
    finally:
        e.close()


def test_grouping_time_is_not_quadratic_in_one_tail(rig):
    """A batch whose records mostly share one tail must not cost much more to group than a uniform one of the same length
    (the bucket path's ranking is quadratic in its fullest bucket, and low bits cannot split one tail)."""
    rows = []
    for L in (MI, 4 * MI):
        rng = np.random.default_rng(L + 3)
        ms = {}
        for dist in ("uniform", "hub-90pct"):
            t = tails_for(dist, L, rng)
            rig.upload_internal(t, at_slide=0)
            _, _, _, taken, _ = rig.e.debug_grouping(path=0)
            ms[dist] = rig.e.time_batch_grouping(reps=5)
            rows.append((L, dist, taken, ms[dist]))
            if dist == "uniform":
                assert taken == BUCKET                 # a uniform batch keeps the hand-written bucket path
        ratio = ms["hub-90pct"] / ms["uniform"]
        rows.append((L, "ratio", 0, ratio))
    print("\n   records  batch       path  grouping ms (ratio: one-tail / uniform)")
    for L, dist, taken, v in rows:
        print(f"  {L:8d}  {dist:10s}  {taken if taken else '':>4}  {v:.4f}")
    for L, dist, _, v in rows:
        if dist == "ratio":
            assert v <= 8.0, f"{L} records, 90 % on one tail: {v:.1f} x the uniform batch's grouping time"


def test_headline_batch_keeps_the_bucket_path():
    """The default workload's batch (soc-LiveJournal1 stand-in, W = 6.9 M stream edges, 69 K edges per batch: 138 K records) is
    grouped by the hand-written bucket path: its hub tails stay far below SU_GRP_MAX_BUCKET records per bucket."""
    from dynamicppr_amd import datagen
    from oracle import oracle as orc
    cfg = datagen.STAND_INS["livejournal"]
    W, c, _, _ = orc.workload_config(cfg.edges, 0.1, 0, 0.01, 100, 0, 0)
    V, e1, e2, _ = datagen.stand_in_stream("livejournal", limit=W + 2 * c)
    g = orc.Graph(V, e1, e2, cfg.directed, W, c)
    e = eng.Engine(V, W, cfg.directed, c)
    try:
        e.load_window(*g.window_edges())
        for _ in range(2):
            assert not g.stream_updates()
            g.inc_construct(1)
            e.set_batch(*g.batch())
            e.slide(*g.new_stream())
            gt, gi, raw, taken, nb = e.debug_grouping(path=0)
            assert len(raw) == 2 * c and taken == BUCKET and nb == buckets(2 * c)
            t = raw.astype(np.int64)
            assert np.bincount(t & (nb - 1)).max() <= SU_GRP_MAX_BUCKET
            assert np.array_equal(gi.astype(np.int64), np.lexsort((np.arange(len(t)), t, t & (nb - 1))))
    finally:
        e.close()
