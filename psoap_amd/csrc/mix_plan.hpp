// mix_plan.hpp -- the pure-host part of the mixture moments (mix_kernels.hpp): the padding of the prediction rows and of
// the sample index, the upper tiles of the rank-S product in launch order, the bytes of every buffer and the argument
// checks.  No HIP call and no HIP header: psoap_gp.hip includes it into the library, and a host compiler builds the same
// text into a stand-alone, sanitized program (tests/host/mix_host_check.cpp).
//
// Rpad = R rounded up to the tile edge (128), Spad = S_max rounded up to the tile engine's K stage (16).  The stacked means
// Mu and their centred, weighted copy D are Spad rows of Rpad doubles: k-major in the sample index, as the tile engine
// takes its operands.  Sbar (full Sigma) and the finished Sigma_mix are Rpad x Rpad; Vbar takes Sbar's place when only the
// variances are accumulated.
#pragma once
#include <vector>

#include "tile_consts.hpp"

namespace psoap {

constexpr int MIX_MAX_S = 4096;          // samples of one mixture (Mu and D: 2 x 8 x 4096 x Rpad bytes)
constexpr int MIX_MAX_R = 1 << 15;       // prediction rows (Rpad^2 stays inside a size_t product of ints)

struct MixTile {
    int ti, tj;      // rows 128 ti .., columns 128 tj .. of Sigma_mix, tj >= ti
};

struct MixPlan {
    int R = 0, S_max = 0, want_sigma = 0;
    int Rpad = 0, Spad = 0, Rt = 0;
    std::vector<MixTile> tiles;          // Rt (Rt + 1) / 2 upper tiles, row-major: the launch order of k_mix_syrk
    long long sbar_doubles = 0;          // Sbar: Rpad^2 with full Sigma, else Vbar: Rpad
    long long out_doubles = 0;           // Sigma_mix: Rpad^2 with full Sigma, else 0
    long long mu_doubles = 0;            // Mu, and as many again for D: Spad x Rpad
    long long small_doubles = 0;         // the weights (Spad), mu_mix, var_within, var_between (Rpad each) and W (one)
    long long bytes = 0;                 // all of it
};

// launch order -> upper tile (row-major over the upper triangle: row ti starts at ti Rt - ti (ti - 1) / 2)
PSOAP_HD inline MixTile mix_tile(int t, int Rt)
{
    int ti = 0;
    while (ti + 1 < Rt && (ti + 1) * Rt - (ti + 1) * ti / 2 <= t) ++ti;
    return MixTile{ti, ti + (t - (ti * Rt - ti * (ti - 1) / 2))};
}

// K-loop depth of a finish over n folded samples
PSOAP_HD inline int mix_depth(int n) { return round_up(n, KB); }

// prediction rows of a predict call of this mode (predict_plan.hpp: Rq)
inline int mix_rows(int mode, int c, int M) { return mode == 0 ? c * M : M; }

// -> nullptr, or why a mixture of R prediction rows and up to S_max samples is refused
inline const char* mix_check_plan(long long R, int S_max, int want_sigma)
{
    if (want_sigma != 0 && want_sigma != 1) return "want_sigma must be 0 (variances only) or 1 (full Sigma)";
    if (R < 1) return "the prediction must have at least 1 row";
    if (R > MIX_MAX_R) return "the prediction must have at most 32768 rows";
    if (S_max < 1) return "S_max must be at least 1";
    if (S_max > MIX_MAX_S) return "S_max must be at most 4096";
    return nullptr;
}

// -> nullptr, or why psoap_chunk_mix_begin is refused (arrays: every required pointer is there)
inline const char* mix_check_begin(int marg, int mode, int c, int M, int S_max, int want_sigma, bool arrays)
{
    if (!arrays) return "bad arguments";
    if (marg != 0 && marg != 1) return "marg must be 0 (the plain conditional) or 1 (under the marginalised continuum)";
    if (mode < 0 || mode > 2 || c < 1 || c > 3 || M < 1) return "mode must be 0, 1 or 2, c 1 .. 3 and M at least 1";
    if (mode == 2 && c != 1) return "mode 2 (predict_f) needs c == 1";
    return mix_check_plan((long long)(mode == 0 ? c : 1) * M, S_max, want_sigma);
}

inline void mix_plan(int R, int S_max, int want_sigma, MixPlan& g)
{
    g = MixPlan();
    g.R = R;
    g.S_max = S_max;
    g.want_sigma = want_sigma;
    g.Rpad = round_up(R, NB);
    g.Spad = round_up(S_max, KB);
    g.Rt = g.Rpad / NB;
    if (want_sigma)
        for (int t = 0; t < g.Rt * (g.Rt + 1) / 2; ++t) g.tiles.push_back(mix_tile(t, g.Rt));
    g.sbar_doubles = want_sigma ? (long long)g.Rpad * g.Rpad : (long long)g.Rpad;
    g.out_doubles = want_sigma ? (long long)g.Rpad * g.Rpad : 0;
    g.mu_doubles = (long long)g.Spad * g.Rpad;
    g.small_doubles = (long long)g.Spad + 3ll * g.Rpad + 1;
    g.bytes = 8 * (g.sbar_doubles + g.out_doubles + 2 * g.mu_doubles + g.small_doubles);
}

// -> nullptr, or why psoap_chunk_mix_add is refused.  weight: finite and > 0
inline const char* mix_check_add(bool active, int n_folded, int S_max, double weight, bool arrays)
{
    if (!arrays) return "bad arguments";
    if (!active)
        return "no mixture on this handle (psoap_chunk_mix_begin first; psoap_chunk_set_data, psoap_chunk_set_baseline and "
               "psoap_chunk_mix_release end one)";
    if (!(weight > 0.0) || weight > 1.7976931348623157e308) return "weight must be finite and > 0";
    if (n_folded >= S_max) return "the mixture already holds S_max samples";
    return nullptr;
}

// -> nullptr, or why psoap_chunk_mix_finish is refused
inline const char* mix_check_finish(bool active, int n_folded, int want_sigma, bool sigma_out, bool arrays)
{
    if (!arrays) return "bad arguments";
    if (!active)
        return "no mixture on this handle (psoap_chunk_mix_begin first; psoap_chunk_set_data, psoap_chunk_set_baseline and "
               "psoap_chunk_mix_release end one)";
    if (sigma_out && !want_sigma) return "Sigma_out must be NULL in the variance-only mode (want_sigma = 0 at psoap_chunk_mix_begin)";
    if (n_folded < 1) return "no sample has been folded yet";
    return nullptr;
}

}  // namespace psoap
