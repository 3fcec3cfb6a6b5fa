"""dppr_assign / dppr_assign_at on the device against the numpy restatement (tests/assign_ref.py) over the dense group_read of
every named group, bit for bit, for host and device destinations.

The rig: V = 777 external ids (three full tiles of 256 and a ragged one), the churn stream of tests/test_renumbering_gpu.py on a
window of 300 edges with renumbering at work (parked and revived vertices; the top of the id range never gets an internal id),
groups of 1, 3, 5, 8, 10 and 16 sources (rows of 2, 4, 6, 8, 10 and 16 doubles: teams of 1, 2, 4, 4, 8 and 8 lanes) and a
target-set group of the five lane kinds of tests/test_targets_gpu.py, all on ONE engine, after 12 group updates."""
import ctypes as C
from itertools import combinations

import numpy as np
import pytest

from dynamicppr_amd import engine as eng
from oracle import oracle as orc
from tests import assign_ref as ref
from tests.assign_ref import bits
from tests.test_export_gpu import Hip
from tests.test_renumbering_gpu import churn_stream
from tests.test_targets_gpu import lane_kinds

pytestmark = pytest.mark.gpu

V, W, CB, EPS, BAND = 777, 300, 30, 1e-9, 120
BATCHES = 12
WIDTHS = (1, 3, 5, 8, 10, 16)
H, D = eng.DEST_HOST, eng.DEST_DEVICE


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free_all()


def same_f(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (tag, got[:6], want[:6])


def same_i(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (tag, got[:8], want[:8])


class Rig:
    def __init__(self, directed, widths=WIDTHS, with_sets=True, batches=BATCHES, seed=5):
        self.directed = directed
        e1, e2 = churn_stream(V, W + 2 * BATCHES * CB + 8 * CB, BAND, seed + directed, back=0.1)
        self.g = g = orc.Graph(V, e1, e2, directed, W, CB)
        self.e = e = eng.Engine(V, W, directed, CB)
        e.set_renumbering(1, growth_pct=8, min_parked=8)
        e.load_window(*g.window_edges())
        first = np.unique(np.concatenate([e1[:W], e2[:W]]))
        rng = np.random.default_rng(99 + directed)
        self.groups, self.sizes = {}, {}     # name -> handle; name -> the number of seeds of every lane
        for n in widths:
            src = [int(x) for x in rng.choice(first, n, replace=False)]
            self.groups[n] = e.add_source_group(src)
            self.sizes[n] = [1] * n
        if with_sets:
            sets = lane_kinds(V, e1, np.random.default_rng(45))
            self.groups["tg"] = e.add_target_group(sets)
            self.sizes["tg"] = [len(s[0]) for s in sets]
        for hd in self.groups.values():
            e.group_init_solve(hd, EPS)
        for _ in range(batches):
            self.step()
        self.read()

    def step(self):
        g, e = self.g, self.e
        assert not g.stream_updates()
        g.inc_construct(1)
        e.set_batch(*g.batch())
        e.slide(*g.new_stream())
        for hd in self.groups.values():
            e.group_update(hd, EPS)

    def read(self):
        """name -> [V][n] p, each column exactly what group_read returns (the reference of every test: read once per state)."""
        self.P = {name: ref.dense(self.e, [hd]) for name, hd in self.groups.items()}

    def classes(self, names):
        return [self.groups[n] for n in names], np.concatenate([self.P[n] for n in names], axis=1)

    def inv_size(self, names):
        return np.array([1.0 / s for n in names for s in self.sizes[n]])


@pytest.fixture(scope="module", params=[1, 0], ids=["directed", "undirected"])
def rig(request):
    r = Rig(request.param)
    yield r
    r.e.close()


class Dev:
    """The device arrays of a caller: label / best / margin / prev [V], three flip lists [V]."""

    def __init__(self, hip):
        self.hip = hip
        self.label, self.prev = hip.alloc(4 * V), hip.alloc(4 * V)
        self.best, self.margin = hip.alloc(8 * V), hip.alloc(8 * V)
        self.lists = tuple(hip.alloc(4 * V) for _ in range(3))

    def get(self, ptr, dtype, n=V):
        return self.hip.read(ptr, np.dtype(dtype).itemsize * n, dtype)

    def set(self, ptr, a):
        a = np.ascontiguousarray(a)
        assert self.hip.L.hipMemcpy(ptr, a.ctypes.data, a.nbytes, 1) == 0


def check_call(e, dev, groups, P, scale, min_score, tag):
    """One call to each destination against the restatement: labels, best, margin, counts."""
    label, best, second, second_label, margin = ref.assign(P, scale, min_score)
    cnt = ref.counts(label, P.shape[1])
    out = e.assign(groups, scale, min_score)
    same_i(out["label"], label, tag + ("label",))
    same_f(out["best"], best, tag + ("best",))
    same_f(out["margin"], margin, tag + ("margin",))
    same_i(out["counts"], cnt, tag + ("counts",))
    assert out["n_flips"] == 0 and out["flips"] is None and int(cnt.sum()) == V
    counts, n_flips = e.assign_dev(groups, dev.label, scale, min_score, dev.best, dev.margin)
    same_i(dev.get(dev.label, np.int32), label, tag + ("label", "device"))
    same_f(dev.get(dev.best, np.float64), best, tag + ("best", "device"))
    same_f(dev.get(dev.margin, np.float64), margin, tag + ("margin", "device"))
    same_i(counts, cnt, tag + ("counts", "device"))
    assert n_flips == 0
    return out


def combos(names):
    pairs = list(combinations(names, 2))
    triples = [(16, "tg", 10), (1, 3, 5), ("tg", 8, 1), (10, 16, 3), (5, "tg", 16)]
    return [(n,) for n in names] + pairs + [t for t in triples if all(x in names for x in t)]


def test_rig_has_every_kind_of_vertex(rig):
    m, sp = rig.e.id_map(), rig.e.id_space()
    print("id space", rig.directed, sp, "never", int(np.count_nonzero(m < 0)))
    assert np.count_nonzero(m < 0) > 0 and sp["parked"] > 0 and sp["revivals"] > 0 and sp["renumberings"] >= 1, sp


def test_labels_best_margin_counts_for_every_combination(rig, hip):
    e, dev = rig.e, Dev(hip)
    names = list(rig.groups)
    seen_unassigned = seen_set_label = 0
    for names_c in combos(names):
        groups, P = rig.classes(names_c)
        n_classes = P.shape[1]
        rng = np.random.default_rng(n_classes)
        zeros = np.where(rng.random(n_classes) < 0.4, 0.0, rng.random(n_classes) + 0.5)
        if n_classes > 1:
            zeros[int(np.argmax(P.sum(axis=0)))] = 0.0     # (the strongest class is among the zero-scaled)
        pos = P[P > 0]
        mid = float(np.median(pos)) if len(pos) else 0.5
        for what, scale in (("null", None), ("ones", np.ones(n_classes)), ("1/|class|", rig.inv_size(names_c)), ("zeros", zeros)):
            for min_score in (0.0, mid, 1e300):
                out = check_call(e, dev, groups, P, scale, min_score, (rig.directed, names_c, what, min_score))
                if what == "zeros":
                    assert not np.any(np.isin(out["label"], np.nonzero(zeros == 0.0)[0])), (names_c, "a zero-scaled class won")
                if min_score == 1e300:
                    assert np.all(out["label"] == -1) and out["counts"][n_classes] == V and not out["best"].any() and not out["margin"].any()
                    assert not np.signbit(out["best"]).any() and not np.signbit(out["margin"]).any()
                if what == "null" and min_score == 0.0:
                    seen_unassigned += int(out["counts"][n_classes])
                    if "tg" in names_c:
                        base = sum(len(rig.sizes[n]) for n in names_c[:names_c.index("tg")])
                        seen_set_label += int(np.count_nonzero(out["label"] >= base))
    assert seen_unassigned > 0 and seen_set_label > 0   # (vertices without an id are unassigned; set lanes do win)


def test_exact_ties_of_a_group_named_twice(rig):
    e = rig.e
    ids = np.arange(V, dtype=np.int32)
    for name, hd in rig.groups.items():
        n = len(rig.sizes[name])
        P = np.concatenate([rig.P[name], rig.P[name]], axis=1)
        out = e.assign([hd, hd])
        label, best, second, second_label, margin = ref.assign(P)
        same_i(out["label"], label, (name, "label"))
        assigned = out["label"] >= 0
        assert assigned.any() and np.all(out["label"] < n), name
        assert np.all(bits(out["margin"][assigned]) == 0), (name, "a tie has the margin +0.0")
        same_f(out["best"], best, (name, "best"))
        at = e.assign_at([hd, hd], ids)
        same_i(at[0], label, (name, "at label"))
        same_i(at[2], second_label, (name, "at second label"))
        # the runner-up is the label's twin in the second naming -- unless another lane of the group itself holds exactly the
        # same score (two symmetric sources of an undirected window do): then the definition makes that smaller class the second
        alone = assigned & ((rig.P[name] == best[:, None]).sum(axis=1) == 1)
        assert 2 * np.count_nonzero(alone) > np.count_nonzero(assigned), name
        assert np.array_equal(at[2][alone], label[alone] + n), name
        assert np.all(at[2][assigned & ~alone] < n), name
        assert np.all(at[2][~assigned] == -1)
    # one class: nothing is second
    hd, P = rig.groups[1], rig.P[1]
    out = e.assign([hd])
    at = e.assign_at([hd], ids)
    assert np.all(at[2] == -1) and np.array_equal(bits(out["margin"]), bits(out["best"])) and np.array_equal(bits(at[3]), bits(at[1]))
    same_i(out["label"], np.where(P[:, 0] > 0, 0, -1).astype(np.int32), "C = 1")


def test_assign_at_equals_the_dense_call(rig):
    e = rig.e
    rng = np.random.default_rng(3)
    every = np.arange(V, dtype=np.int32)
    dup = rng.integers(0, V, 1000).astype(np.int32)      # duplicates, no order
    for names_c in [(1,), (3,), (8,), (16,), ("tg",), (10, "tg"), (5, 16, "tg"), (1, 3)]:
        groups, P = rig.classes(names_c)
        for scale in (None, rig.inv_size(names_c)):
            for min_score in (0.0, 1e-4):
                label, best, second, second_label, margin = ref.assign(P, scale, min_score)
                out = e.assign(groups, scale, min_score)
                for ids in (every, dup, every[::-1][:5]):
                    al, ab, a2, am = e.assign_at(groups, ids, scale, min_score)
                    tag = (names_c, scale is None, min_score, len(ids))
                    same_i(al, out["label"][ids], tag)
                    same_f(ab, out["best"][ids], tag)
                    same_f(am, out["margin"][ids], tag)
                    same_i(a2, second_label[ids], tag)
                    same_f(am, margin[ids], tag)   # (margin = best - second: the runner-up's score is held through it)
        # m = 0: a no-op that writes nothing
        L = eng.lib()
        g = np.array(groups, dtype=np.int32)
        lab = np.full(2, -7, dtype=np.int32)
        ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        assert L.dppr_assign_at(e._h, g.ctypes.data_as(ip), len(g), None, 0.0, None, 0, lab.ctypes.data_as(ip), None, None, None) == 0
        assert np.all(lab == -7)
        assert all(len(x) == 0 for x in e.assign_at(groups, np.empty(0, dtype=np.int32)))


def test_flips_against_the_previous_batch(hip):
    """Labels before and after a batch on the churn rig (a 10-source group and the set group; parked and revived vertices)."""
    rig = Rig(1, widths=(10, 3), batches=BATCHES)
    e, dev = rig.e, Dev(hip)
    names_c = (10, "tg", 3)
    groups, P0 = rig.classes(names_c)
    before = e.assign(groups)["label"]
    same_i(before, ref.assign(P0)[0], "before")
    first = e.assign(groups, prev=np.full(V, -1, dtype=np.int32))        # against all -1: every assigned vertex flips
    want = ref.flips(np.full(V, -1, dtype=np.int32), before)
    assert first["n_flips"] == len(want[0]) == np.count_nonzero(before >= 0)
    for a, b in zip(first["flips"], want):
        same_i(a, b, "against all -1")
    sp0 = e.id_space()
    for _ in range(3):
        rig.step()
    rig.read()
    sp1 = e.id_space()
    print("flips rig", sp0, sp1)
    groups, P1 = rig.classes(names_c)
    after = ref.assign(P1)[0]
    fid, fold, fnew = ref.flips(before, after)
    n = len(fid)
    assert n >= 2, n                                                       # (otherwise the test shows nothing)
    cnt = ref.counts(after, P1.shape[1])
    # host destination: a prev of its own, then in place
    out = e.assign(groups, prev=before)
    assert out["n_flips"] == n and out["label"] is not before
    same_i(out["label"], after, "after")
    same_i(out["counts"], cnt, "counts with prev")
    for a, b in zip(out["flips"], (fid, fold, fnew)):
        same_i(a, b, "host flips")
    mine = before.copy()
    out = e.assign(groups, prev=mine, inplace=True)
    assert out["label"] is mine and out["n_flips"] == n
    same_i(mine, after, "in place")
    for a, b in zip(out["flips"], (fid, fold, fnew)):
        same_i(a, b, "host flips in place")
    # cap = 0 counts only; cap = n - 1 writes nothing; cap = n writes exactly the list
    out = e.assign(groups, prev=before, cap=0)
    assert out["n_flips"] == n and out["flips"] is None
    lists = tuple(np.full(n + 3, -9, dtype=np.int32) for _ in range(3))
    out = e.assign(groups, prev=before, cap=n - 1, lists=lists)
    assert out["n_flips"] == n and out["flips"] is None and all(np.all(a == -9) for a in lists)
    same_i(out["label"], after, "labels of a call whose lists did not fit")
    out = e.assign(groups, prev=before, cap=n, lists=lists)
    assert out["n_flips"] == n
    for a, b in zip(lists, (fid, fold, fnew)):
        same_i(a[:n], b, "cap = n")
        assert np.all(a[n:] == -9)
    # device destination: the same, with prev a second array and prev = label
    sent = np.full(V, -9, dtype=np.int32)
    for inplace in (False, True):
        for cap, fits in ((0, False), (n - 1, False), (n, True), (V + 5, True)):
            for ptr in dev.lists:
                dev.set(ptr, sent)
            prev_ptr = dev.label if inplace else dev.prev
            dev.set(prev_ptr, before)
            counts, nf = e.assign_dev(groups, dev.label, prev_ptr=prev_ptr, cap=cap, flip_ptrs=dev.lists if cap else (None, None, None))
            assert nf == n, (inplace, cap)
            same_i(counts, cnt, ("device counts", inplace, cap))
            same_i(dev.get(dev.label, np.int32), after, ("device label", inplace, cap))
            if not inplace:
                same_i(dev.get(dev.prev, np.int32), before, "prev is only read")
            for ptr, b in zip(dev.lists, (fid, fold, fnew)):
                got = dev.get(ptr, np.int32)
                if fits:
                    same_i(got[:n], b, ("device flips", inplace, cap))
                    assert np.all(got[n:] == -9)
                else:
                    assert np.all(got == -9), ("nothing is written when the flips do not fit", inplace, cap)
    # no flips against itself
    out = e.assign(groups, prev=after)
    assert out["n_flips"] == 0 and all(len(a) == 0 for a in out["flips"])
    e.close()


def test_rejections_leave_everything_untouched(rig, hip):
    e, L = rig.e, eng.lib()
    dev = Dev(hip)
    short_i, short_d = hip.alloc(4 * V - 4), hip.alloc(8 * V - 8)
    ip, dp, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    g16, g3 = rig.groups[16], rig.groups[3]
    good = np.array([g16, g3], dtype=np.int32)
    bad_g = np.array([g16, 77], dtype=np.int32)
    neg_g = np.array([-1], dtype=np.int32)
    many = np.array([g16] * 17, dtype=np.int32)
    label, best, margin = np.full(V, -7, dtype=np.int32), np.full(V, 2.5), np.full(V, 3.5)
    counts, nf = np.full(258, -5, dtype=np.int64), np.full(1, -5, dtype=np.int64)
    prev = np.full(V, -1, dtype=np.int32)
    lists = [np.full(V, -9, dtype=np.int32) for _ in range(3)]
    ones = np.ones(19)

    def scale_with(x):
        s = ones.copy()
        s[18] = x
        return s

    def untouched():
        host = np.all(label == -7) and np.all(best == 2.5) and np.all(margin == 3.5) and np.all(counts == -5) and np.all(nf == -5) and \
            all(np.all(a == -9) for a in lists) and np.all(prev == -1)
        devs = [hip.read(p, nb) for p, nb in ((dev.label, 4 * V), (dev.best, 8 * V), (dev.margin, 8 * V), (dev.prev, 4 * V), (short_i, 4 * V - 4),
                                              (short_d, 8 * V - 8))] + [hip.read(p, 4 * V) for p in dev.lists]
        return host and all(np.all(x == 0xAB) for x in devs)

    def call(groups=good, n_groups=None, scale=None, min_score=0.0, dest=H, out_label=label.ctypes.data, out_best=best.ctypes.data,
             out_margin=margin.ctypes.data, out_counts=counts, prev_label=prev.ctypes.data, cap=V, fl=tuple(a.ctypes.data for a in lists), handle=None):
        return L.dppr_assign(e._h if handle is None else handle, groups.ctypes.data_as(ip) if groups is not None else None,
                             len(groups) if n_groups is None else n_groups, scale.ctypes.data_as(dp) if scale is not None else None, min_score, dest,
                             out_label, out_best, out_margin, out_counts.ctypes.data_as(i64p) if out_counts is not None else None, prev_label, cap,
                             nf.ctypes.data_as(i64p), *fl)

    nan, inf = float("nan"), float("inf")
    dl = dict(dest=D, out_label=dev.label, out_best=dev.best, out_margin=dev.margin, prev_label=dev.prev, fl=dev.lists)
    bad = [dict(groups=bad_g), dict(groups=neg_g), dict(groups=None, n_groups=1), dict(n_groups=0), dict(n_groups=-1), dict(groups=many),
           dict(scale=scale_with(-1e-300)), dict(scale=scale_with(inf)), dict(scale=scale_with(nan)), dict(min_score=-1e-300), dict(min_score=nan),
           dict(dest=2), dict(dest=-1), dict(out_label=None), dict(out_counts=None), dict(cap=-1),
           dict(fl=(None, lists[1].ctypes.data, lists[2].ctypes.data)), dict(fl=(lists[0].ctypes.data, None, lists[2].ctypes.data)),
           dict(fl=(lists[0].ctypes.data, lists[1].ctypes.data, None)),
           # a device destination: a host pointer, an allocation one element short, a misaligned pointer -- for every array
           dict(dl, out_label=label.ctypes.data), dict(dl, out_best=best.ctypes.data), dict(dl, out_margin=margin.ctypes.data),
           dict(dl, prev_label=prev.ctypes.data), dict(dl, fl=(lists[0].ctypes.data, dev.lists[1], dev.lists[2])),
           dict(dl, fl=(dev.lists[0], dev.lists[1], lists[2].ctypes.data)),
           dict(dl, out_label=short_i), dict(dl, out_best=short_d), dict(dl, out_margin=short_d), dict(dl, prev_label=short_i),
           dict(dl, fl=(dev.lists[0], short_i, dev.lists[2])),
           dict(dl, out_label=dev.label + 2), dict(dl, out_best=dev.best + 4), dict(dl, out_margin=dev.margin + 4), dict(dl, prev_label=dev.prev + 2),
           dict(dl, fl=(dev.lists[0] + 2, dev.lists[1], dev.lists[2]), cap=V - 1),
           dict(dl, out_label=dev.label + 4), dict(dl, out_best=dev.best + 8)]      # (aligned, and one element too short)
    for kw in bad:
        assert call(**kw) == -1, {k: v for k, v in kw.items() if k != "fl"}
        assert untouched(), kw.keys()
    assert call(handle=C.c_void_p()) == -1 and untouched()
    # a short list is fine when cap says so (cap entries, not V), and so is a NULL best / margin
    assert call(**dict(dl, fl=(dev.lists[0], short_i, dev.lists[2]), cap=V - 1, out_best=None, out_margin=None)) == 0
    # assign_at
    ids, at_l, at_b = np.array([0, V - 1], dtype=np.int32), np.full(2, -7, dtype=np.int32), np.full(2, 2.5)
    at2, atm = np.full(2, -7, dtype=np.int32), np.full(2, 3.5)

    def call_at(groups=good, n_groups=None, scale=None, min_score=0.0, ids=ids, m=2, out_label=at_l, handle=None):
        return L.dppr_assign_at(e._h if handle is None else handle, groups.ctypes.data_as(ip) if groups is not None else None,
                                len(groups) if n_groups is None else n_groups, scale.ctypes.data_as(dp) if scale is not None else None, min_score,
                                ids.ctypes.data_as(ip) if ids is not None else None, m, out_label.ctypes.data_as(ip) if out_label is not None else None,
                                at_b.ctypes.data_as(dp), at2.ctypes.data_as(ip), atm.ctypes.data_as(dp))

    for kw in [dict(groups=bad_g), dict(groups=None, n_groups=1), dict(n_groups=0), dict(groups=many), dict(scale=scale_with(-1.0)), dict(scale=scale_with(nan)),
               dict(min_score=-1.0), dict(min_score=nan), dict(ids=np.array([0, V], dtype=np.int32)), dict(ids=np.array([-1, 0], dtype=np.int32)),
               dict(ids=None), dict(m=-1), dict(out_label=None), dict(handle=C.c_void_p())]:
        assert call_at(**kw) == -1, kw.keys()
        assert np.all(at_l == -7) and np.all(at_b == 2.5) and np.all(at2 == -7) and np.all(atm == 3.5), kw.keys()
    # the Python layer refuses a scale of the wrong length before the library is called
    with pytest.raises(eng.DpprError, match="one entry per class"):
        e.assign([g16, g3], scale=np.ones(5))
    # 16 groups of 16 lanes are the 256 classes: accepted
    out = e.assign([g16] * 16)
    assert len(out["counts"]) == 257 and out["counts"].sum() == V and np.all(out["label"] < 16)


def test_device_time_is_reported_with_profiling_on(rig):
    e = rig.e
    e.set_profiling(1)
    try:
        groups, P = rig.classes((10, "tg"))
        e.assign(groups, prev=np.full(V, -1, dtype=np.int32))
        ms = e.query_ms()
        assert ms is not None and 0.0 < ms < 100.0, ms
        e.assign_at(groups, np.arange(50, dtype=np.int32))
        ms = e.query_ms()
        assert ms is not None and 0.0 < ms < 100.0, ms
    finally:
        e.set_profiling(0)
