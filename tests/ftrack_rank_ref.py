"""The ranked, position and sample queries over a forward track (dppr_ftrack_topk_ranked / _rank_score_at / _position_at / _sample,
include/dppr.h) in numpy, for the tests: a thin glue over tests/rank_ref.py, tests/position_ref.py and tests/sample_ref.py. The
inputs are the track's columns BY EXTERNAL ID and complete (the p of tests/ftrack_ref.py's columns, or a dense read) -- a vertex
without an internal id keeps its own p, it is not 0 -- the out-CSR of the track's epoch by external id (read_out_graph), and the
seeds of every column as external ids (the ids of its start set, whatever their weights). A vertex without a row has out-degree 0
and no neighbour; a seed is excluded under SEEDS whether or not it has a row."""
import numpy as np

from tests import position_ref, rank_ref, sample_ref

NONE, DEV, DEG, INV_DEG = rank_ref.NONE, rank_ref.DEV, rank_ref.DEG, rank_ref.INV_DEG
SEEDS, IN_NEIGHBOURS, OUT_NEIGHBOURS = rank_ref.SEEDS, rank_ref.IN_NEIGHBOURS, rank_ref.OUT_NEIGHBOURS


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Graph:
    """The stored edges of an epoch by external id, from its out-CSR (row [V + 1], col)."""

    def __init__(self, V, row, col):
        self.V = int(V)
        self.tails, self.heads = rank_ref.edges(row, col)
        self.outdeg = rank_ref.out_degree(self.V, self.tails)


def scores(cols, seeds, graph=None, factor=NONE, g=None, allow=None, deny=None, exclude=0):
    """The score of every column by external id: a list of [V] arrays. cols: the p of every column, [V] each, by external id;
    seeds: one array of external ids per column; graph: a Graph (needed by DEG / INV_DEG and the neighbour flags alone)."""
    V = len(cols[0])
    excl = None
    if exclude:
        if exclude & (IN_NEIGHBOURS | OUT_NEIGHBOURS):
            excl = rank_ref.excluded(V, graph.tails, graph.heads, seeds, exclude)
        else:   # (the seeds alone: no graph is looked at)
            none = np.zeros(0, dtype=np.int64)
            excl = rank_ref.excluded(V, none, none, seeds, exclude)
    outdeg = graph.outdeg if factor in (DEG, INV_DEG) else None
    return rank_ref.scores(cols, factor, outdeg=outdeg, g=g, allow=allow, deny=deny, excl=excl)


def topk(s, k, min_score=0.0):
    return rank_ref.topk(s, k, min_score)


def positions(score_list, ids, min_score=0.0):
    """(pos int32 [len(ids)][m], counts int32 [m])"""
    return position_ref.group_positions(score_list, ids, min_score)


def sample(score_list, S, min_score=0.0, seed=0, first=0):
    """(ids [m][S], w [m][S], total [m], support [m], status [m]): the lane index of a draw is the column."""
    return sample_ref.group_sample(np.stack(score_list, axis=1), S, min_score, seed, first)
