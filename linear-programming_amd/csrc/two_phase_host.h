// two_phase_host.h -- the RULE of the step between the phases of n-solve-tableau (src/simplex.lisp:405-434), once,
// for every host copy of it: double (mi355x_two_phase_handover, the members of mi355x_multibatch_two_phase_handover),
// float (mi355x_stab_solve_two_phase) and the exact integers (mi355x_xtab_solve_two_phase).  Host-only: no HIP header,
// no exported symbol (tests/two_phase_check.cpp builds it with the host compiler alone).  How a row comes back, what
// "is zero" means and how a forced pivot is issued are the caller's lambdas; everything around the rule -- handles,
// member views, the hand-over proper (:437-451) -- stays at the call sites.
//
// NOT this rule: cp_drive_out (capi_colpart.inc) assembles the row from column shards, takes the lowest global column
// across them and stops on negative elements of compact shards -- another algorithm around the same two /= 0 tests;
// and the device forms k_sb_between / k_xb_between, which run the step inside a kernel.
#pragma once
#include "../../include/mi355x_simplex.h"

#include <algorithm>
#include <cstdint>
#include <vector>

// (fp= 0 objective factor), :405-407, in T: |0 - objective| <= threshold; a NaN objective is not feasible
template <class T> inline bool tp_feasible(T objective, T threshold)
{
    const T d = T(0) - objective;
    return (d < T(0) ? -d : d) <= threshold;
}

// :425-431: the lowest main column j < num_vars with an exact non-zero entry in `row` that is not basic, or -1
template <class T, class IsZero>
inline int64_t tp_entering_column(const T *row, int64_t num_vars, const int64_t *basis, int64_t m, IsZero is_zero)
{
    for (int64_t j = 0; j < num_vars; ++j)
        if (!is_zero(row[j]) && std::find(basis, basis + m, j) == basis + m) return j;
    return -1;
}

// :419-434: every artificial variable still basic (basis[i] >= num_vars), in row order, is pivoted out on the column
// above.  fetch_row(i, row) fills `row` with row i AS THE PIVOTS BEFORE IT LEFT IT; pivot(col, i) makes the forced
// pivot; on_pivot() counts it at once, so that an early return leaves the pivots already made counted.  `basis` (m
// entries, the host's copy) is kept up to date.  MI_OK, MI_ART_NONZERO (row i's RHS is not an exact zero),
// MI_ART_STUCK (no column qualifies), or whatever fetch_row / pivot returned other than MI_OK.
template <class T, class IsZero, class FetchRow, class Pivot, class OnPivot>
inline int tp_drive_out(int64_t m, int64_t num_vars, int64_t rhs_index, int64_t *basis, IsZero is_zero,
                        FetchRow fetch_row, Pivot pivot, OnPivot on_pivot)
{
    std::vector<T> row;
    for (int64_t i = 0; i < m; ++i) {
        if (basis[i] < num_vars) continue;
        int rc = fetch_row(i, row);
        if (rc != MI_OK) return rc;
        if (!is_zero(row[(size_t)rhs_index])) return MI_ART_NONZERO;
        const int64_t col = tp_entering_column(row.data(), num_vars, basis, m, is_zero);
        if (col < 0) return MI_ART_STUCK;
        rc = pivot(col, i);
        if (rc != MI_OK) return rc;
        basis[i] = col;
        on_pivot();
    }
    return MI_OK;
}
