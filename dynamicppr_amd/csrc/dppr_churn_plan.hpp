// dppr_churn_plan.hpp -- what a change of a running source group's sources does to its interleaved rows: the new source
// count, row width and lane split, which old lane every new lane takes its column from, and whether the rows have to be
// re-interleaved or the sweep groups re-cut. Pure host code without HIP includes (dppr_engine.hip plans
// dppr_group_replace_source / dppr_group_add_source / dppr_group_remove_source with it and launches dppr_churn.hpp;
// tests/native/churn_test.cpp drives it on the CPU against a plain restatement).
#pragma once

namespace dppr {

constexpr int CHURN_LANES = 16; // sources a group holds at most (GS_MAX of dppr_multi.hpp, asserted equal in dppr_churn.hpp)

// row geometry of a group (the same functions as row_width / row_spl of dppr_multi.hpp, asserted equal in dppr_churn.hpp)
constexpr int churn_row_width(int n_sources, bool full_rows) {
    return full_rows ? (n_sources > 8 ? 16 : 8) : n_sources <= 2 ? 2 : (n_sources + 1) / 2 * 2;
}
constexpr int churn_row_spl(int gw) { return gw > 8 ? 2 : 1; }

enum ChurnOp { CHURN_REPLACE = 0, CHURN_ADD = 1, CHURN_REMOVE = 2 };

struct ChurnPlan {
    bool ok = false;       // the operation is admissible (index in range, room for one more, more than one left)
    int n = 0;             // sources afterwards
    int gw = 0, spl = 0;   // doubles per row afterwards, doubles per lane of an octet
    int lane = -1;         // the lane that is initialised and solved from scratch (-1: none, CHURN_REMOVE)
    bool relayout = false; // p / r are re-interleaved through map[] (another width, or lanes that shift)
    bool recut = false;    // the first group of more than 8 doubles per row: sweep groups of at most 512 vertices from now on
    int map[CHURN_LANES] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1}; // new lane -> old lane; -1: zeros
                           // (padding, lanes beyond the row, and the lane that is about to be initialised)
};

// n sources on rows of gw doubles now (gw as the group was created: full_rows = the DPPR_GROUP_FULL_ROWS layout);
// index: the lane replaced / removed (ignored by CHURN_ADD, whose new source takes lane n); wide: a group with
// rows of more than 8 doubles exists already.
inline ChurnPlan churn_plan(ChurnOp op, int n, int gw, int index, bool full_rows, bool wide) {
    ChurnPlan pl;
    if (n < 1 || n > CHURN_LANES) return pl;
    if (op == CHURN_ADD ? n >= CHURN_LANES : (index < 0 || index >= n)) return pl;
    if (op == CHURN_REMOVE && n <= 1) return pl;
    pl.ok = true;
    pl.n = op == CHURN_ADD ? n + 1 : op == CHURN_REMOVE ? n - 1 : n;
    pl.gw = churn_row_width(pl.n, full_rows);
    pl.spl = churn_row_spl(pl.gw);
    pl.lane = op == CHURN_ADD ? n : op == CHURN_REPLACE ? index : -1;
    // survivors keep their order: a removal moves the lanes behind it down by one
    const int survivors = op == CHURN_REMOVE ? n - 1 : n;
    for (int j = 0; j < survivors; ++j) pl.map[j] = op == CHURN_REMOVE && j >= index ? j + 1 : j;
    if (op == CHURN_REPLACE) pl.map[index] = -1;
    pl.relayout = op == CHURN_REMOVE || pl.gw != gw;
    pl.recut = pl.spl == 2 && !wide;
    return pl;
}

} // namespace dppr
