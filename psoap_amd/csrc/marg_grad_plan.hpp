// marg_grad_plan.hpp -- the pure-host part of the gradient of the continuum-marginalised likelihood
// (marg_grad_kernels.hpp): argument validation, the column layout of the [K | I | Ht] workspace, every appended tile
// column's first non-zero block row and the launches of every block row.  No HIP call and no HIP header:
// psoap_gp.hip includes it into the library, and a host compiler builds the same text into a stand-alone, sanitized
// program (tests/host/marg_grad_host_check.cpp).  marg_plan.hpp is used as it is.
//
// Layout.  One matrix is Npad rows of ld = 2 Npad + 128 Q doubles: K's P tile columns, then the P tile columns of I at
// tile column P (where the plain gradient keeps them: k_grad_alpha_partial and the first K loop of the contraction
// address W_I = U^-T as they always did), then the Q tile columns of Ht at tile column 2 P, in marg_plan.hpp's slot
// order (ascending first row).  Appended column a = 0 .. P + Q - 1 counts I's tile columns, then H's in the column
// order of H; tile[a] is where it lives, first[a] the first block row that can be non-zero (j for I_j, the plan's
// first row for a tile column of H; P: none).  Nothing above it is read or written.
//
// Block row p.  The active appended columns are I_0 .. I_p -- contiguous with the rest of K's block row, tile columns
// p .. P + p, as in the plain gradient -- and the slots 0 .. active[p] - 1 of Ht at tile columns 2 P ..: two ranges.
// The choice made here is TWO STRIP LAUNCHES per block row (k_trsm_strip over tile columns p + 1 .. P + p, then over
// 2 P .. 2 P + active[p] - 1) and ONE update launch whose blocks 0 .. P take the first range and the others the second
// (marg_grad_update_tile).  The alternative -- I and Ht merged in ascending order of first row, one launch, a column map
// for every kernel that addresses W_I -- would move W_I away from where k_grad_alpha_partial, the contraction and the
// finishing sums expect it; two more small launches per block row cost less than a second set of those kernels.
#pragma once
#include <stddef.h>

#include <vector>

#include "marg_plan.hpp"

namespace psoap {

// the bounds of a group of matrices (grad_kernels.hpp: GRAD_GROUP_MAX, GRAD_WS_BYTES; marg_grad_kernels.hpp asserts it)
constexpr int MARG_GRAD_GROUP_MAX = 8;
constexpr size_t MARG_GRAD_WS_BYTES = (size_t)1 << 30;

struct MargGradRow {
    int update_k, update_h;      // blocks of the update launch: tile columns p .. P + p, then 2 P .. 2 P + update_h - 1
    int strip_k, strip_h;        // blocks of the two strip launches: tile columns p + 1 .. P + p; 2 P .. 2 P + strip_h - 1
};

struct MargGradPlan {
    int N = 0, P = 0, Q = 0;
    int ld = 0;                          // doubles per row of the workspace
    int tile_I = 0, tile_H = 0;          // first tile column of I and of Ht
    std::vector<int> tile, first;        // per appended column (I_0 .. I_{P-1}, H_0 .. H_{Q-1})
    std::vector<MargGradRow> rows;       // per block row
};

// the tile column block x of block row p's update launch works on (x < update_k + update_h)
PSOAP_HD inline int marg_grad_update_tile(int p, int x, int P) { return x <= P ? p + x : 2 * P + (x - P - 1); }

// doubles of one matrix's workspace
inline size_t marg_grad_matrix_doubles(int Npad, int Q) { return (size_t)Npad * (2 * (size_t)Npad + (size_t)NB * Q); }

// matrices per group of a call: grad_group_size's rule with the Ht columns counted
inline int marg_grad_group_size(int B, int Npad, int Q)
{
    const size_t per = sizeof(double) * marg_grad_matrix_doubles(Npad, Q);
    size_t g = MARG_GRAD_WS_BYTES / per;
    if (g < 1) g = 1;
    if (g > (size_t)MARG_GRAD_GROUP_MAX) g = MARG_GRAD_GROUP_MAX;
    return B < (int)g ? B : (int)g;
}

// -> nullptr, or why a call is refused (the messages of psoap_chunk_lnlike_marg for the baseline)
inline const char* marg_grad_check(int B, int c, bool have_baseline, bool stale_weight)
{
    if (B < 1) return "B must be at least 1";
    if (c < 1 || c > 3) return "number of components must be 1, 2 or 3";
    if (!have_baseline) return "call psoap_chunk_set_baseline first";
    if (stale_weight)
        return "psoap_chunk_set_data changed the data the baseline's weights were given for (psoap_chunk_set_baseline again)";
    return nullptr;
}

// ---- the time-variable kernel under the baseline (psoap_chunk_lnlike_marg_tv, _marg_tv_grad, psoap_chunk_fisher_marg_tv) ----
// What the three entries are called with, as far as a refusal can depend on it: no pointer is read.
enum class MargTvEntry { Value, Grad, Fisher };
struct MargTvCall {
    bool arrays;                          // the required arrays are there (Grad: grad_gp is not one of them)
    bool grad_gp, grad_tau, grad_rest;    // Grad: grad_gp, grad_tau, and grad_lwl or grad_mu, are there
    int B, c, T;                          // Value, Grad: B;  Fisher: T
    int max_batch, max_T;                 // Value: B <= max_batch;  Fisher: T <= max_T (FISHER_MAX_T of fisher_kernels.hpp)
    bool have_times, open_stream, have_baseline, stale_weight;
};

// -> nullptr, or why a call is refused, in this order: the arrays; (Grad) the NULL rules of psoap_chunk_lnlike_tv_grad; c;
// B or T; the handle's state as the time-variable entries ask for it -- times set, no open stream -- and then as the marginal
// entries do, with the messages of psoap_chunk_lnlike_marg: a baseline, and not a stale one.  A tau that is no time scale is
// not a refusal: like a negative hyper-parameter it gives -inf / NaN, after the call.  The caller puts the entry's name in front.
inline const char* marg_tv_check(MargTvEntry entry, const MargTvCall& a)
{
    if (!a.arrays) return "bad arguments";
    if (entry == MargTvEntry::Grad) {
        if (!a.grad_gp && (a.grad_tau || a.grad_rest))
            return "grad_gp == NULL asks for the value only: grad_tau, grad_lwl and grad_mu must be NULL too";
        if (a.grad_gp && !a.grad_tau) return "grad_tau goes with grad_gp";
    }
    if (a.c < 1 || a.c > 3) return "number of components must be 1, 2 or 3";
    if (entry == MargTvEntry::Value && (a.B < 1 || a.B > a.max_batch)) return "batch size outside [1, max_batch]";
    if (entry == MargTvEntry::Grad && a.B < 1) return "B must be at least 1";
    if (entry == MargTvEntry::Fisher && (a.T < 1 || a.T > a.max_T)) return "the number of tangents must be between 1 and 32";
    if (!a.have_times) return "call psoap_chunk_set_times first";
    if (a.open_stream) return "the handle has an open stream (psoap_stream_close first)";
    return marg_grad_check(1, a.c, a.have_baseline, a.stale_weight);
}

// ---- time scales on the batch route (psoap_batch_set_tau) -------------------------------------------------------------------
// -> nullptr, or why the call is refused, in this order: the array; c; B; the handle's state in the words of the time-variable
// entries -- times set, no open stream -- and no baseline: the value under one goes through psoap_chunk_lnlike_marg_tv; then a
// pending upload (psoap_batch_upload, _upload_velocities or _upload_orbits) and its B and c.  A tau that is
// no time scale is not a refusal: the evaluation gives -inf for that proposal.  The caller puts the entry's name in front.
inline const char* batch_tau_check(bool array, int B, int c, bool pending, int pend_B, int pend_c, bool have_times,
                                   bool open_stream, bool have_baseline)
{
    if (!array) return "bad arguments";
    if (c < 1 || c > 3) return "number of components must be 1, 2 or 3";
    if (B < 1) return "B must be at least 1";
    if (!have_times) return "call psoap_chunk_set_times first";
    if (open_stream) return "the handle has an open stream (psoap_stream_close first)";
    if (have_baseline)
        return "the handle has a baseline (psoap_chunk_set_baseline): the value under a baseline goes through "
               "psoap_chunk_lnlike_marg_tv";
    if (!pending) return "no upload is pending (psoap_batch_upload, psoap_batch_upload_velocities or psoap_batch_upload_orbits first)";
    if (B != pend_B || c != pend_c) return "B and c must be those of the pending upload";
    return nullptr;
}

// ---- lnprob(p) under the time-variable kernel (psoap_chunk_lnprob_tv_grad, psoap_chunk_lnprob_marg_tv_grad) -----------------
// -> nullptr, or why the call is refused before the orbits are looked at: the arrays; the NULL rules of
// psoap_chunk_lnlike_tv_grad (grad_gp == NULL: the value only, and then grad_orb, grad_tau, grad_vel and grad_mu are NULL too;
// grad_orb and grad_tau go with grad_gp); B; the grid and the dates; times set, no open stream.  `who` is not needed: the caller
// puts the entry's name in front.  The baseline is asked for (marg) or refused (plain) after the orbits, by the caller.
inline const char* lnprob_tv_check(bool arrays, bool grad_gp, bool grad_orb, bool grad_tau, bool grad_rest, int B, bool have_grid,
                                   bool have_times, bool open_stream)
{
    if (!arrays) return "bad arguments";
    if (!grad_gp && (grad_orb || grad_tau || grad_rest))
        return "grad_gp == NULL asks for the value only: grad_orb, grad_tau, grad_vel and grad_mu must be NULL too";
    if (grad_gp && !(grad_orb && grad_tau)) return "grad_orb and grad_tau go with grad_gp";
    if (B < 1) return "B must be at least 1";
    if (!have_grid) return "call psoap_chunk_set_grid and psoap_chunk_set_dates first";
    if (!have_times) return "call psoap_chunk_set_times first";
    if (open_stream) return "the handle has an open stream (psoap_stream_close first)";
    return nullptr;
}

inline void marg_grad_plan(const MargPlan& pl, MargGradPlan& out)
{
    out = MargGradPlan();
    const int P = pl.P, Q = pl.Q;
    out.N = pl.N;
    out.P = P;
    out.Q = Q;
    out.ld = 2 * NB * P + NB * Q;
    out.tile_I = P;
    out.tile_H = 2 * P;
    for (int j = 0; j < P; ++j) {
        out.tile.push_back(out.tile_I + j);
        out.first.push_back(j);
    }
    for (int t = 0; t < Q; ++t) {
        out.tile.push_back(out.tile_H + pl.slot[(size_t)t]);
        out.first.push_back(pl.first[(size_t)t]);
    }
    for (int p = 0; p < P; ++p) {
        const int act = pl.active[(size_t)p];
        out.rows.push_back(MargGradRow{p > 0 ? P + 1 : 0, p > 0 ? act : 0, P, act});
    }
}

}  // namespace psoap
