"""CPU references for the Chebyshev flux calibration (tests/test_calibration_reference.py, tests/test_gpu_calibration.py).

    B = K(fixed) + sigma_fixed^2,  C = K(cal, fixed),  A = K(cal) + sigma_cal^2      (sums over the components)
    fl' = mu + C B^-1 (fl_fixed - mu),  C' = A - C B^-1 C^T
    D[i][k] = fl_cal[i] T_k(u_i),  u = (2 x - (a + b)) / (b - a) on [a, b] = [lwl0, lwl1],  k = 0 .. order
    X = (D^T C'^-1 D)^-1 D^T C'^-1 fl',  fl_cor = D X

``calibrate_ext`` does all of it in np.longdouble, from the grids (the blocks formed in long double) or from caller-given
float64 A, B, C (the explicit ABI): the oracle's long-double fills, Cholesky and forward substitution, a Chebyshev recurrence
on u and a back-substitution.  ``calibrate_f64`` is the float64 evaluation of the same formulas (oracle.calibration_blocks +
oracle.optimize_calibration: SciPy's cho_factor / cho_solve, numpy's Chebyshev with its ``off + scl * x`` map of the
abscissa).  ``calibrate_f64_route`` is float64 as well but goes the device's way (W = U^-T C^T, fl' = mu + W^T z,
C' = A - W^T W) and takes the seeded defects of tests/test_calibration_reference.py.

``cycle_ext`` / ``cycle_chunk_ext`` are the loops of covariance.cycle_calibration / cycle_calibration_chunk over the
long-double solve (the flux stays long double from solve to solve); ``cycle_f64`` / ``cycle_chunk_f64`` their float64 twins.

Run as a script it prints, per case and entry level (and for the static form's problem where c = 1), the error of the float64
evaluation against the long-double one, and the same for the two cycles: the table from which tests/test_gpu_calibration.py takes its bounds.
"""
from __future__ import annotations

import functools
import os
import sys
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), ROOT, os.path.dirname(os.path.abspath(__file__)),
           os.path.join(ROOT, "tests", "golden")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from psoap_amd import synthetic as syn  # noqa: E402

_LD = np.longdouble
NB = 128           # the device's tile; a block row of B
SLAB = 256         # rows of W that one block of the transposed GEMV sums

OUTPUTS = ("fl_cor", "X")
LEVELS = ("grids", "blocks")


@dataclass
class Cal:
    fl_cor: np.ndarray
    X: np.ndarray
    flp: np.ndarray = None      # fl', the conditional mean at the epoch's pixels
    Cp: np.ndarray = None       # C', the conditional covariance


# ---- the cases -------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    c: int
    M: int
    N: int
    order: int
    mu: float
    n_epochs: int
    n_pix: int
    limit_array: int
    seed: int
    masked_fraction: float = 0.0
    n_fixed: int = None         # keep only the first pixels of the reference epochs (M > N)
    scale: float = 1.04


# Each the smallest shape at which the named thing can go wrong (Npad, Mpad: N, M rounded up to the tile of 128):
CASES = (
    Case("a", 1, 9, 9, 0, 1.0, 2, 9, 1, 971),                  # everything inside one tile, constant correction
    Case("b", 1, 128, 128, 15, 1.0, 2, 128, 1, 974),           # exact tiles, no padding rows, highest order: columns 16 and
                                                               # 17 of the augmented tile
    Case("c", 2, 129, 258, 5, 1.0, 3, 129, 2, 972),            # one pixel into the second tile in both passes
    Case("d", 1, 127, 381, 8, 0.97, 4, 127, 3, 975),           # one short of a tile; mu != 1 through the right-hand side and m0
    Case("e", 2, 257, 257, 15, 1.0, 2, 257, 1, 976),           # three block rows in pass 2; Npad = 384: a half-filled second slab
    Case("f", 3, 200, 800, 2, 1.0, 5, 200, 4, 973),            # three components, seven block rows in pass 1
    Case("g", 2, 130, 60, 3, 1.02, 2, 130, 1, 977, n_fixed=60),      # M > N: two augmented column tiles on one block row
    Case("h", 2, 140, 410, 4, 1.0, 4, 150, 3, 978, masked_fraction=0.1),   # M, N at no special value, unequal epochs
    Case("i", 1, 171, 513, 15, 1.0, 4, 171, 3, 979),           # Npad = 640: three slabs, the last half-filled
)


def case_id(case):
    return f"{case.name}-c{case.c}-M{case.M}-N{case.N}-o{case.order}"


def case_named(name):
    return next(c for c in CASES if c.name == name)


def first_pixels(inputs, n_fixed):
    """the same problem against the first ``n_fixed`` reference pixels only (M > N when the epoch is longer)"""
    out = dict(inputs)
    out.update(lwls_fixed=np.ascontiguousarray(inputs["lwls_fixed"][:, :n_fixed]), fl_fixed=inputs["fl_fixed"][:n_fixed].copy(),
               sigma_fixed=inputs["sigma_fixed"][:n_fixed].copy())
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(case) -> dict:
    """epoch 0 of a synthetic chunk against the next ``limit_array`` epochs (make_golden_host.cal_case), read-only"""
    from make_golden_host import cal_case
    inp = cal_case(syn, case.c, case.n_epochs, case.n_pix, case.seed, case.masked_fraction, case.scale,
                   limit_array=case.limit_array)
    if case.n_fixed is not None:
        inp = first_pixels(inp, case.n_fixed)
    inp = {k: (np.ascontiguousarray(v, dtype=np.float64) if isinstance(v, np.ndarray) else float(v)) for k, v in inp.items()}
    assert (inp["lwl_cal"].shape[0], inp["fl_fixed"].shape[0]) == (case.M, case.N), \
        (case.name, inp["lwl_cal"].shape[0], inp["fl_fixed"].shape[0])
    for v in inp.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return inp


def static_inputs(inputs) -> dict:
    """optimize_calibration_static's reading of the same arrays: the Chebyshev abscissa is the kernel abscissa too"""
    assert np.atleast_2d(inputs["lwls_fixed"]).shape[0] == 1
    out = dict(inputs)
    out["lwls_cal"] = np.ascontiguousarray(np.asarray(inputs["lwl_cal"])[None, :])
    return out


# ---- long double -------------------------------------------------------------------------------------------------------
def blocks_ext(inputs):
    """A, B, C in long double from the float64 grids, sigmas and gp"""
    import oracle
    cal = np.atleast_2d(np.asarray(inputs["lwls_cal"], dtype=np.float64))
    fix = np.atleast_2d(np.asarray(inputs["lwls_fixed"], dtype=np.float64))
    gp = np.asarray(inputs["gp"], dtype=np.float64)
    A, B = oracle._sym_ext(cal, gp), oracle._sym_ext(fix, gp)
    A[np.diag_indices_from(A)] += np.asarray(inputs["sigma_cal"], dtype=_LD) ** 2
    B[np.diag_indices_from(B)] += np.asarray(inputs["sigma_fixed"], dtype=_LD) ** 2
    C = sum(oracle._fill_ext(cal[k], fix[k], gp[2 * k], gp[2 * k + 1]) for k in range(cal.shape[0]))
    return A, B, C


def cheb_u_ext(lwl0, lwl1, x):
    a, b = _LD(lwl0), _LD(lwl1)
    return (_LD(2) * np.asarray(x, dtype=_LD) - (a + b)) / (b - a)


def cheb_ext(u, order):
    """T_k(u), k = 0 .. order, by the three-term recurrence in long double -> (len(u), order + 1)"""
    u = np.asarray(u, dtype=_LD)
    T = np.empty((u.shape[0], order + 1), dtype=_LD)
    T[:, 0] = _LD(1)
    if order >= 1:
        T[:, 1] = u
    for k in range(2, order + 1):
        T[:, k] = _LD(2) * u * T[:, k - 1] - T[:, k - 2]
    return T


def _bsolve_ext(L, y):
    """L^-T y by back-substitution (long double)"""
    x = np.array(y, dtype=_LD)
    for i in range(L.shape[0] - 1, -1, -1):
        if i + 1 < L.shape[0]:
            x[i] -= L[i + 1:, i] @ x[i + 1:]
        x[i] /= L[i, i]
    return x


def solve_ext(lwl0, lwl1, lwl_cal, fl_cal, fl_fixed, A, B, C, order=1, mu=1.0) -> Cal:
    """the solve from given blocks, every step in long double (the flux vectors may be long double already)"""
    import oracle
    A, B, C = (np.asarray(m, dtype=_LD) for m in (A, B, C))
    fl_cal = np.asarray(fl_cal, dtype=_LD)
    L1 = oracle._chol_ext(B)
    W = oracle._fsolve_ext(L1, C.T)                                             # (N, M)
    z = oracle._fsolve_ext(L1, np.asarray(fl_fixed, dtype=_LD).reshape(-1) - _LD(mu))
    flp = _LD(mu) + W.T @ z
    Cp = A - W.T @ W
    D = fl_cal[:, None] * cheb_ext(cheb_u_ext(lwl0, lwl1, lwl_cal), order)
    W2 = oracle._fsolve_ext(oracle._chol_ext(Cp), np.concatenate([D, flp[:, None]], axis=1))
    G = W2.T @ W2
    n = order + 1
    L3 = oracle._chol_ext(G[:n, :n])
    X = _bsolve_ext(L3, oracle._fsolve_ext(L3, G[:n, n]))
    return Cal(D @ X, X, flp, Cp)


def calibrate_ext(inputs, order=1, mu=1.0, blocks=None) -> Cal:
    """``inputs``: the dict of ``case_inputs``.  Without ``blocks`` A, B, C are formed in long double from the grids;
    with ``blocks = (A, B, C)`` the caller's float64 matrices are taken as they are (the explicit ABI)."""
    A, B, C = blocks_ext(inputs) if blocks is None else blocks
    return solve_ext(inputs["lwl0"], inputs["lwl1"], inputs["lwl_cal"], inputs["fl_cal"], inputs["fl_fixed"], A, B, C,
                     order, mu)


# ---- float64 -----------------------------------------------------------------------------------------------------------
def blocks_f64(inputs):
    import oracle
    return oracle.calibration_blocks(inputs["lwls_cal"], inputs["sigma_cal"], inputs["lwls_fixed"], inputs["sigma_fixed"],
                                     inputs["gp"])


def calibrate_f64(inputs, order=1, mu=1.0, blocks=None) -> Cal:
    """the float64 evaluation of the same formulas: the oracle's fills and its SciPy solve"""
    import oracle
    A, B, C = blocks_f64(inputs) if blocks is None else blocks
    fl_cor, X = oracle.optimize_calibration(inputs["lwl0"], inputs["lwl1"], inputs["lwl_cal"], inputs["fl_cal"],
                                            inputs["fl_fixed"], A, B, C, order=order, mu_GP=mu)
    return Cal(fl_cor, X)


def design_f64(lwl0, lwl1, lwl_cal, fl_cal, order, last_factor=2.0):
    """D as the device builds it: numpy's map ``off + scl * x`` of the abscissa, then the recurrence.  ``last_factor``
    is the 2 of T_order = 2 u T_(order-1) - T_(order-2) (a seeded defect replaces it)"""
    scl = 2.0 / (lwl1 - lwl0)
    off = (-lwl1 - lwl0) / (lwl1 - lwl0)
    u = off + scl * np.asarray(lwl_cal, dtype=np.float64)
    T = np.empty((u.shape[0], order + 1))
    T[:, 0] = 1.0
    if order >= 1:
        T[:, 1] = u
    for k in range(2, order + 1):
        T[:, k] = (last_factor if k == order else 2.0) * u * T[:, k - 1] - T[:, k - 2]
    return np.asarray(fl_cal, dtype=np.float64)[:, None] * T


def calibrate_f64_route(inputs, order=1, mu=1.0, blocks=None, D=None, cbc_rows=None, flp_rows=None) -> Cal:
    """float64 the device's way: W = U^-T C^T and z = U^-T (fl_fixed - mu) from one factor of B, fl' = mu + W^T z,
    C' = A - W^T W, then the normal equations from U2^-T [D | fl'].  ``D`` replaces the design matrix; ``cbc_rows`` /
    ``flp_rows`` keep only the first rows of W in C B^-1 C^T / in fl' (the seeded defects)."""
    from scipy.linalg import cho_factor, cho_solve, cholesky, solve_triangular
    A, B, C = blocks_f64(inputs) if blocks is None else blocks
    if D is None:
        D = design_f64(inputs["lwl0"], inputs["lwl1"], inputs["lwl_cal"], inputs["fl_cal"], order)
    U = cholesky(B, lower=False)
    W = solve_triangular(U, C.T, trans="T", lower=False)
    z = solve_triangular(U, np.asarray(inputs["fl_fixed"], dtype=np.float64).reshape(-1) - mu, trans="T", lower=False)
    rf = W.shape[0] if flp_rows is None else flp_rows
    rc = W.shape[0] if cbc_rows is None else cbc_rows
    flp = mu + W[:rf].T @ z[:rf]
    Cp = A - W[:rc].T @ W[:rc]
    W2 = solve_triangular(cholesky(Cp, lower=False), np.concatenate([D, flp[:, None]], axis=1), trans="T", lower=False)
    G = W2.T @ W2
    n = order + 1
    X = cho_solve(cho_factor(G[:n, :n]), G[:n, n])
    return Cal(D @ X, X, flp, Cp)


def errors(got, ref) -> dict:
    """fl_cor relative to max|ref fl_cor|, X relative to max|ref X|; ``got`` a Cal or a (fl_cor, X) pair"""
    if not isinstance(got, Cal):
        got = Cal(*got)

    def rel(a, b):
        a, b = np.asarray(a, dtype=_LD), np.asarray(b, dtype=_LD)
        assert a.shape == b.shape, (a.shape, b.shape)
        return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))

    return {"fl_cor": rel(got.fl_cor, ref.fl_cor), "X": rel(got.X, ref.X)}


def stage_errors(got, ref) -> dict:
    """the same measure on every intermediate both sides hold (fl', C'), for failure messages"""
    out = {}
    for k in ("flp", "Cp"):
        a, b = getattr(got, k), getattr(ref, k)
        if a is not None and b is not None:
            out[k] = float(np.max(np.abs(np.asarray(a, dtype=_LD) - b)) / np.max(np.abs(b)))
    return out


# ---- references of the cases, and the float64 table ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_blocks(case):
    """the float64 A, B, C handed to the explicit form, read-only"""
    blocks = tuple(np.ascontiguousarray(m) for m in blocks_f64(case_inputs(case)))
    for m in blocks:
        m.setflags(write=False)
    return blocks


@functools.lru_cache(maxsize=None)
def case_ext(case, level="grids") -> Cal:
    blocks = None if level == "grids" else case_blocks(case)
    return calibrate_ext(case_inputs(case), case.order, case.mu, blocks)


@functools.lru_cache(maxsize=None)
def static_ext(case) -> Cal:
    return calibrate_ext(static_inputs(case_inputs(case)), case.order, case.mu)


def measure_f64():
    """-> [(case id, {level: errors})]: ``grids`` and ``blocks`` for every case, ``static`` (the problem
    optimize_calibration_static poses with the same arrays, from its grids) for the one-component cases"""
    rows = []
    for case in CASES:
        inp = case_inputs(case)
        f = calibrate_f64(inp, case.order, case.mu)
        err = {lv: errors(f, case_ext(case, lv)) for lv in LEVELS}
        if case.c == 1:
            err["static"] = errors(calibrate_f64(static_inputs(inp), case.order, case.mu), static_ext(case))
        rows.append((case_id(case), err))
    return rows


def max_row(rows, level):
    return {k: max(r[1][level][k] for r in rows if level in r[1]) for k in OUTPUTS}


# ---- the cycles ----------------------------------------------------------------------------------------------------------
CYCLE_EPOCHS, CYCLE_PIX, CYCLE_N, CYCLE_ORDER, CYCLE_LIMIT = 5, 90, 2, 1, 3
CYCLE_GP = (0.1, 10.0)


@functools.lru_cache(maxsize=None)
def cycle_case():
    """-> (lwl, fl, sigma, mask, truth): five epochs of one sinusoidal spectrum with per-epoch flux scales, and a 10 % mask"""
    rng = np.random.RandomState(4)
    n_ep, n_pix = CYCLE_EPOCHS, CYCLE_PIX
    lwl = np.tile(np.linspace(8.5560, 8.5568, n_pix), (n_ep, 1)) + 1e-6 * rng.standard_normal((n_ep, 1))
    truth = 1.0 + 0.08 * np.sin(2e4 * (lwl - 8.556))
    scale = np.array([1.0, 1.08, 0.93, 1.05, 0.97])[:, None]
    fl = truth * scale + 0.004 * rng.standard_normal((n_ep, n_pix))
    sigma = np.full_like(fl, 0.004)
    mask = rng.uniform(size=fl.shape) > 0.1
    for a in (lwl, fl, sigma, mask, truth):
        a.setflags(write=False)
    return lwl, fl, sigma, mask, truth


def _static_dict(wl0, wl1, wl_cal, fl_cal, sigma_cal, wl_fixed, fl_fixed, sigma_fixed, amp, l):
    return dict(lwl0=wl0, lwl1=wl1, lwl_cal=wl_cal, lwls_cal=np.asarray(wl_cal)[None, :], fl_cal=fl_cal, sigma_cal=sigma_cal,
                lwls_fixed=np.asarray(wl_fixed).reshape(1, -1), fl_fixed=np.asarray(fl_fixed).reshape(-1),
                sigma_fixed=np.asarray(sigma_fixed).reshape(-1), gp=np.array([amp, l]))


def _cycle(solve, T, wl, fl, sigma, mask, amp, l, ncycles, order, limit_array, mu, cheb_all):
    """the loop of covariance.cycle_calibration (mask None) / cycle_calibration_chunk in the number type ``T``;
    solve(inputs dict) -> Cal, cheb_all(wl0, wl1, x, X) -> the polynomial on every pixel of an epoch"""
    wl, sigma = np.asarray(wl, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    wl0, wl1 = np.min(wl), np.max(wl)
    fl_out = np.array(fl, dtype=T)
    for _ in range(ncycles):
        for i in range(wl.shape[0]):
            rest = [np.delete(a, i, axis=0)[0:limit_array] for a in (wl, fl_out, sigma)]
            if mask is None:
                inp = _static_dict(wl0, wl1, wl[i], fl_out[i], sigma[i], *rest, amp, l)
                fl_out[i] = solve(inp).fl_cor
            else:
                mt, mr = mask[i], np.delete(mask, i, axis=0)[0:limit_array]
                inp = _static_dict(wl0, wl1, wl[i][mt], fl_out[i][mt], sigma[i][mt], *[a[mr] for a in rest], amp, l)
                fl_out[i] = fl_out[i] * cheb_all(wl0, wl1, wl[i], solve(inp).X)
    return fl_out


def _chebval_ext(wl0, wl1, x, X):
    return cheb_ext(cheb_u_ext(wl0, wl1, x), X.shape[0] - 1) @ X


def _chebval_f64(wl0, wl1, x, X):
    from numpy.polynomial import chebyshev as npcheb
    return npcheb.chebval((2.0 * x - (wl0 + wl1)) / (wl1 - wl0), X)


def _chebval_f64_mapped(wl0, wl1, x, X):
    """the polynomial on the solve's own ``off + scl * x`` abscissa instead (what D X uses)"""
    return design_f64(wl0, wl1, x, np.ones_like(x), X.shape[0] - 1) @ X


def cycle_ext(wl, fl, sigma, amp, l, ncycles, order=1, limit_array=3, mu=1.0):
    return _cycle(lambda inp: calibrate_ext(inp, order, mu), _LD, wl, fl, sigma, None, amp, l, ncycles, order, limit_array,
                  mu, None)


def cycle_f64(wl, fl, sigma, amp, l, ncycles, order=1, limit_array=3, mu=1.0):
    return _cycle(lambda inp: calibrate_f64(inp, order, mu), np.float64, wl, fl, sigma, None, amp, l, ncycles, order,
                  limit_array, mu, None)


def cycle_chunk_ext(wl, fl, sigma, mask, amp, l, ncycles, order=1, limit_array=3, mu=1.0):
    return _cycle(lambda inp: calibrate_ext(inp, order, mu), _LD, wl, fl, sigma, mask, amp, l, ncycles, order, limit_array,
                  mu, _chebval_ext)


def cycle_chunk_f64(wl, fl, sigma, mask, amp, l, ncycles, order=1, limit_array=3, mu=1.0, cheb_all=_chebval_f64):
    return _cycle(lambda inp: calibrate_f64(inp, order, mu), np.float64, wl, fl, sigma, mask, amp, l, ncycles, order,
                  limit_array, mu, cheb_all)


def cycle_error(got, ref):
    """max |got - ref| relative to max |ref| over the whole block"""
    return float(np.max(np.abs(np.asarray(got, dtype=_LD) - ref)) / np.max(np.abs(ref)))


@functools.lru_cache(maxsize=None)
def cycle_refs():
    """-> (cycle_ext, cycle_chunk_ext) of ``cycle_case``"""
    lwl, fl, sigma, mask, _ = cycle_case()
    args = (*CYCLE_GP, CYCLE_N, CYCLE_ORDER, CYCLE_LIMIT)
    return cycle_ext(lwl, fl, sigma, *args), cycle_chunk_ext(lwl, fl, sigma, mask, *args)


def measure_cycles():
    """-> {"cycle", "chunk": float64 twin against long double; "chunk_map": the float64 chunk cycle with the polynomial on
    the solve's mapped abscissa against the one with the host's form of u}"""
    lwl, fl, sigma, mask, _ = cycle_case()
    args = (*CYCLE_GP, CYCLE_N, CYCLE_ORDER, CYCLE_LIMIT)
    ref, ref_chunk = cycle_refs()
    f_chunk = cycle_chunk_f64(lwl, fl, sigma, mask, *args)
    f_mapped = cycle_chunk_f64(lwl, fl, sigma, mask, *args, cheb_all=_chebval_f64_mapped)
    return {"cycle": cycle_error(cycle_f64(lwl, fl, sigma, *args), ref), "chunk": cycle_error(f_chunk, ref_chunk),
            "chunk_map": cycle_error(f_mapped, f_chunk.astype(_LD))}


if __name__ == "__main__":
    rows = measure_f64()
    cols = [(lv, k) for lv in LEVELS + ("static",) for k in OUTPUTS]
    print(f"{'case':20s} " + " ".join(f"{lv + ':' + k:>13s}" for lv, k in cols))
    for name, err in rows:
        print(f"{name:20s} " + " ".join(f"{err[lv][k]:13.2e}" if lv in err else f"{'-':>13s}" for lv, k in cols))
    print(f"{'max':20s} " + " ".join(f"{max_row(rows, lv)[k]:13.2e}" for lv, k in cols))
    cyc = measure_cycles()
    print(f"{'cycle':20s} {cyc['cycle']:13.2e}")
    print(f"{'cycle_chunk':20s} {cyc['chunk']:13.2e}   (mapped abscissa against the host's u: {cyc['chunk_map']:.2e})")
