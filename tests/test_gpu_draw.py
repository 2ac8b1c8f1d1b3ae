"""GPU tests of the posterior draws (psoap_chunk_predict_draw, psoap_draw_normals; psoap_amd/csrc/draw_kernels.hpp,
draw_plan.hpp, draw_rng.hpp).

Shapes: N = 300 (10 epochs x 30 pixels of psoap_amd.synthetic), the prediction rows R across the 128-tile edges through
(c, M) = (1, 127), (1, 128), (1, 129), (2, 64), (2, 65), (3, 43), (1, 257), in the modes each is defined for (mode 2 with one
component, modes 0 and 1 with two, mode 0 with three: the sum of three components needs M == N).

The mean.  Sigma does not depend on the flux, and with a flux equal to the offset the conditional mean is the prior mean
exactly.  The factor and the product are therefore tested on the chunk's wavelengths and noise with a constant flux and
prior means 0 (mu == 0 bit for bit, asserted), where out - mu IS the product: with mu of order one, out = fl(product + mu)
keeps the product only to 2^-53 |out|, which no implementation can undo and the bounds below have no room for.  That the
mean of the real flux is added, and added once with one rounding, is a test of its own: out(real flux) == out(constant
flux) + mu bit for bit.

Orientation.  The call returns X[d, :] = mu + U^T z_d; with z = I_R row d is mu plus ROW d of U, so the lower factor of
A = Sigma + nugget I is L = (out - mu)^T, and L L^T = U^T U = A.  "Lower triangular with exact zeros above the diagonal"
is therefore exact zeros BELOW the diagonal of out - mu.

Bounds (none fitted to the device's results):
* the factor: |L L^T - A|_ij <= 4 (R + 2) 2^-53 sqrt(A_ii A_jj), the backward error of a Cholesky factorisation in any
  summation order (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.3) with a factor 4 for the subtraction
  of mu, at nugget 1e-8 and 1e-4;
* the product: |(out - mu) - L z| <= (R + 2) 2^-53 (|L| |z|) entrywise, L from the identity call;
* the generator: relative error against the long-double evaluation of the same Box-Muller formula (draw_reference.normals)
  at most 8 times the largest one measured on the device for psoap_draw_normals(seed 20260101, 4, 2^18)
  (profiles/predict_draw.md: GENERATOR_MEASURED below); moments over the 2^20 values within 6 standard errors;
* end to end: D = 4096 seeded draws at (c, M) = (2, 65): every entry of the sample covariance about mu within
  6 sqrt((A_ii A_jj + A_ij^2) / D) of A_ij, the sample mean within 6 sqrt(A_ii / D) of mu.
"""
import ctypes
import functools

import numpy as np
import pytest

import draw_reference as dr
from psoap_amd import synthetic as syn

pytestmark = pytest.mark.gpu

LD = np.longdouble
U53 = 2.0 ** -53
# (c, M, mode)
CASES = [(1, 127, 2), (1, 128, 2), (1, 129, 2), (2, 64, 0), (2, 64, 1), (2, 65, 0), (2, 65, 1), (3, 43, 0), (1, 257, 2)]
IDS = [f"c{c}-M{M}-mode{m}" for c, M, m in CASES]
NUGGETS = (1e-8, 1e-4)
SEED = 20260101
GENERATOR_MEASURED = 3.68e-16      # largest relative error of the device's normals, measured once (profiles/predict_draw.md)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def chunk(c):
    return syn.make_chunk(c, 10, 30, seed=4100 + c)


def _args(c, M, mode, zero_mean=False):
    ch = chunk(c)
    pred = np.linspace(ch.lwls[0].min(), ch.lwls[0].max(), M)
    mus = [0.0] * c if (mode == 0 or zero_mean) else [1.0]
    return mode, ch.lwls, np.stack([pred] * c), mus, list(syn.GP_BASE[c])


def _offset(c, mode):
    """what the library subtracts from the flux with prior means 0 (include/psoap_gp.h: psoap_predict)"""
    return 1.0 if (mode == 0 or (mode == 1 and c == 2)) else 0.0


def _handle(c, flux=None):
    from psoap_amd.chunk import ChunkHandle
    ch = chunk(c)
    return ChunkHandle(ch.fl if flux is None else np.full_like(ch.fl, flux), ch.sigma)


@functools.lru_cache(maxsize=None)
def device(case):
    """one handle per case, once per session: mu, Sigma, the identity calls at both nuggets, the product calls"""
    c, M, mode = case
    rng = np.random.default_rng(77 + 1000 * c + M)
    with _handle(c, flux=_offset(c, mode)) as h:
        mu, Sigma = h.predict(*_args(*case, zero_mean=True))
        R = mu.shape[0]
        assert np.all(mu == 0.0)
        out = {"mu": mu, "Sigma": Sigma, "R": R, "eye": {g: h.predict_draw(R, z=np.eye(R), nugget=g) for g in NUGGETS}}
        zs = {D: rng.standard_normal((D, R)) for D in (1, 5, 129)}
        spike = 1e-9 * rng.standard_normal((2, R))
        spike[0, R // 3] = 1e9
        spike[1, R - 1] = -1e9
        zs["spike"] = spike
        out["z"] = zs
        out["prod"] = {k: h.predict_draw(z.shape[0], z=z) for k, z in zs.items()}
    return out


def _factor_residual(dev, nugget):
    """-> (L, the largest |L L^T - A|_ij / (sqrt(A_ii A_jj) 2^-53 (R + 2)))"""
    R = dev["R"]
    A = dev["Sigma"].astype(LD) + LD(nugget) * np.eye(R, dtype=LD)
    L = (dev["eye"][nugget].astype(LD) - dev["mu"].astype(LD)[None, :]).T
    d = np.sqrt(np.diag(A))
    return L, float(np.max(np.abs(dr.gram(L) - A) / np.outer(d, d)) / (U53 * (R + 2)))


@pytest.mark.parametrize("nugget", NUGGETS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_factor(case, nugget):
    dev = device(case)
    R = dev["R"]
    assert dev["eye"][nugget].shape == (R, R) and np.all(np.isfinite(dev["eye"][nugget]))
    upper = dev["eye"][nugget] - dev["mu"][None, :]
    assert np.all(np.tril(upper, -1) == 0.0), "out - mu has entries below the diagonal: a K-loop past tj or an unmasked tile"
    L, worst = _factor_residual(dev, nugget)
    print(f"factor {case} nugget {nugget:g}: max |L L^T - A| / (sqrt(A_ii A_jj) (R + 2) 2^-53) = {worst:.3f} (bound 4)")
    assert np.all(np.diag(L) > 0)
    assert worst <= 4.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_product(case):
    dev = device(case)
    R, mu = dev["R"], dev["mu"].astype(LD)
    L = (dev["eye"][NUGGETS[0]].astype(LD) - mu[None, :]).T
    for key, z in dev["z"].items():
        got = dev["prod"][key].astype(LD) - mu[None, :]
        want = z.astype(LD) @ L.T
        scale = np.abs(z).astype(LD) @ np.abs(L).T
        worst = float(np.max(np.abs(got - want) / scale) / (U53 * (R + 2)))
        print(f"product {case} z {key}: max |out - mu - L z| / ((R + 2) 2^-53 |L||z|) = {worst:.3f} (bound 1)")
        assert worst <= 1.0, key


@pytest.mark.parametrize("case", [(1, 129, 2), (2, 65, 0), (2, 64, 1)], ids=["c1-M129-mode2", "c2-M65-mode0", "c2-M64-mode1"])
def test_mean_of_the_real_flux_is_added_with_one_rounding(case):
    dev = device(case)
    c = case[0]
    with _handle(c) as h:
        mu, Sigma = h.predict(*_args(*case))
        assert _same_bits(Sigma, dev["Sigma"]) and np.max(np.abs(mu)) > 1e-2
        for key, z in dev["z"].items():
            assert _same_bits(h.predict_draw(z.shape[0], z=z), dev["prod"][key] + mu[None, :]), key


def test_determinism_and_indexing():
    case = (2, 65, 0)
    with _handle(2) as h:
        h.predict(*_args(*case))
        a = h.predict_draw(8, seed=SEED)
        assert _same_bits(a, h.predict_draw(8, seed=SEED))
        assert not np.any(a == h.predict_draw(8, seed=SEED + 1))
        assert _same_bits(a[:3], h.predict_draw(3, seed=SEED))
        R = a.shape[1]
        from psoap_amd import _lib
        z = np.empty((8, R))
        _lib.check(_lib.load().psoap_draw_normals(h.device, ctypes.c_ulonglong(SEED), 8, R, _lib.dptr(z)), "psoap_draw_normals")
        assert _same_bits(a, h.predict_draw(8, z=z))
        # element i of draw d does not depend on the number of elements either
        z2 = np.empty((3, 7))
        _lib.check(_lib.load().psoap_draw_normals(h.device, ctypes.c_ulonglong(SEED), 3, 7, _lib.dptr(z2)), "psoap_draw_normals")
        assert _same_bits(z2, z[:3, :7])


def test_draw_after_predict_marg_uses_the_marginal_sigma():
    case = (2, 65, 0)
    ch = chunk(2)
    with _handle(2) as h:
        h.set_baseline(1, ch.lwl, ch.epoch_index, ch.n_epochs, [0.05, 0.02])
        mu_p, Sig_p = h.predict(*_args(*case))
        mu_m, Sig_m = h.predict_marg(*_args(*case))
        R = mu_m.shape[0]
        eye = h.predict_draw(R, z=np.eye(R))
    dev = {"R": R, "mu": mu_m, "Sigma": Sig_m, "eye": {1e-8: eye}}
    _, worst = _factor_residual(dev, 1e-8)
    dev["Sigma"] = Sig_p
    _, plain = _factor_residual(dev, 1e-8)
    print(f"marginal: residual against the marginal Sigma {worst:.3f}, against the plain one {plain:.3e} (bound 4)")
    assert worst <= 4.0 < plain


@functools.lru_cache(maxsize=None)
def generated():
    from psoap_amd import _lib
    z = np.empty((4, 2 ** 18))
    _lib.check(_lib.load().psoap_draw_normals(_lib.default_device(), ctypes.c_ulonglong(SEED), 4, 2 ** 18, _lib.dptr(z)),
               "psoap_draw_normals")
    return z


def test_generator_values():
    z = generated()
    want = dr.normals(SEED, 4, 2 ** 18)
    assert np.all(np.isfinite(z))
    rel = np.abs(z.astype(LD) - want) / np.abs(want)
    rel[want == 0] = np.where(z[want == 0] == 0.0, 0.0, np.inf)
    print(f"generator: largest relative error against long double {float(rel.max()):.3e} (measured once: {GENERATOR_MEASURED:.3e})")
    assert float(rel.max()) <= 8 * GENERATOR_MEASURED


def test_generator_moments():
    z = generated().ravel()
    n = z.size
    se = {"mean": (z.mean(), 0.0, np.sqrt(1.0 / n)), "variance": (np.mean(z * z), 1.0, np.sqrt(2.0 / n)),
          "fourth": (np.mean(z ** 4), 3.0, np.sqrt(96.0 / n)), "lag1": (np.mean(z[:-1] * z[1:]), 0.0, np.sqrt(1.0 / n))}
    for name, (got, want, s) in se.items():
        print(f"generator {name}: {got:.6f} (expected {want}, standard error {s:.2e}, {abs(got - want) / s:.2f} s.e.)")
        assert abs(got - want) <= 6 * s, name


def test_end_to_end_statistics():
    case, D = (2, 65, 0), 4096
    with _handle(2) as h:
        mu, Sigma = h.predict(*_args(*case))
        x = h.predict_draw(D, seed=SEED)
    A = Sigma + 1e-8 * np.eye(mu.shape[0])
    r = x - mu[None, :]
    cov = r.T @ r / D
    d = np.diag(A)
    c_dev = np.max(np.abs(cov - A) / np.sqrt((np.outer(d, d) + A * A) / D))
    m_dev = np.max(np.abs(x.mean(axis=0) - mu) / np.sqrt(d / D))
    print(f"end to end: covariance {c_dev:.2f}, mean {m_dev:.2f} standard errors at the worst entry (bound 6)")
    assert c_dev <= 6.0 and m_dev <= 6.0


def test_refusals():
    from psoap_amd import _lib
    L = _lib.load()
    case = (2, 64, 1)
    ch = chunk(2)

    def refused(h, *a):
        out = np.empty((8, 64))
        st = ctypes.c_int(-9)
        rc = L.psoap_chunk_predict_draw(h._h, *a, _lib.dptr(out), ctypes.byref(st))
        return rc, L.psoap_last_error().decode()

    no_sigma = "psoap_chunk_predict_draw: no predict call has formed Sigma on this handle"
    with _handle(2) as h:
        assert refused(h, 5, ctypes.c_ulonglong(1), None, 1e-8) == (2, no_sigma + " (psoap_chunk_predict or "
                                                                    "psoap_chunk_predict_marg with Sigma_out first)")
        h.predict(*_args(*case))
        assert h.predict_draw(5, seed=1).shape == (5, 64)
        for D in (0, -1):
            assert refused(h, D, ctypes.c_ulonglong(1), None, 1e-8) == (2, "psoap_chunk_predict_draw: D must be at least 1")
        for g in (-1e-12, np.inf, np.nan):
            assert refused(h, 5, ctypes.c_ulonglong(1), None, g) == (2, "psoap_chunk_predict_draw: nugget must be finite and >= 0")
        # the calls that form no Sigma clear the record; so do a release and a change of the data or the baseline
        clear = [lambda: h.predict(*_args(*case), want_sigma="diag"), lambda: h.predict(*_args(*case), want_sigma=False),
                 h.predict_release, lambda: h.set_data(ch.fl, ch.sigma),
                 lambda: h.set_baseline(1, ch.lwl, ch.epoch_index, ch.n_epochs, [0.05, 0.02])]
        for f in clear:
            h.predict(*_args(*case))
            assert h.predict_draw(1, seed=1).shape == (1, 64)
            f()
            rc, msg = refused(h, 5, ctypes.c_ulonglong(1), None, 1e-8)
            assert rc == 2 and msg.startswith(no_sigma)
            with pytest.raises(_lib.PsoapError):
                h.predict_draw(5, seed=1)
        h.predict(*_args(*case))
        h.stream_open(2)
        try:
            assert refused(h, 5, ctypes.c_ulonglong(1), None, 1e-8) == (
                2, "psoap_chunk_predict_draw: the handle has an open stream (psoap_stream_close first)")
        finally:
            h.stream_close()
        with pytest.raises(ValueError):
            h.predict_draw(5)
        with pytest.raises(ValueError):
            h.predict_draw(5, seed=1, z=np.zeros((5, 64)))
        with pytest.raises(ValueError):
            h.predict_draw(5, z=np.zeros((5, 63)))


def test_status_one_on_a_rank_one_sigma():
    """129 identical prediction ln-wavelengths, no baseline, nugget 0: Sigma is exactly rank one, the second pivot is
    0 or a rounding error of either sign -- where it is not positive the call reports status 1 with NaN everywhere"""
    from psoap_amd import _lib
    ch = chunk(1)
    pred = np.full((1, 129), ch.lwls[0].mean())
    with _handle(1) as h:
        h.predict(2, ch.lwls, pred, [1.0], list(syn.GP_BASE[1]))
        out = np.zeros((3, 129))
        st = ctypes.c_int(-9)
        rc = _lib.load().psoap_chunk_predict_draw(h._h, 3, ctypes.c_ulonglong(1), None, 0.0, _lib.dptr(out), ctypes.byref(st))
        assert rc == 0 and st.value == 1 and np.all(np.isnan(out))
        with pytest.raises(np.linalg.LinAlgError):
            h.predict_draw(3, seed=1, nugget=0.0)
        assert h.predict_draw(3, seed=1, nugget=1e-8).shape == (3, 129)      # the same Sigma, still resident


def _chunk2d(s):
    from psoap_amd import data as pdata

    def full(v, fill):
        out = np.full(s.mask.shape, fill)
        out[s.mask] = v
        return out
    date = np.broadcast_to(s.dates[:, None], s.mask.shape).copy()
    return pdata.Chunk(np.exp(full(s.lwl, 8.5)), full(s.fl, 1.0), full(s.sigma, 1.0), date, s.mask.copy())


def test_python_layer(tmp_path):
    from psoap_amd import covariance, retrieve
    from psoap_amd.utils import registered_params
    s = syn.make_chunk(3, 6, 24, seed=883, masked_fraction=0.1)
    p_orb = syn.make_orbit_proposals("ST3", 1, seed=884)[0]
    pars = dict(zip(registered_params["ST3"], list(p_orb) + list(syn.GP_BASE[3])))
    M = 2 * s.n_pix
    base = retrieve.retrieve_components("ST3", _chunk2d(s), pars)
    zero = retrieve.retrieve_components("ST3", _chunk2d(s), pars, n_draws=0, seed=5)
    assert list(base) == list(zero) and all(_same_bits(base[k], zero[k]) for k in base)
    res = retrieve.retrieve_components("ST3", _chunk2d(s), pars, n_draws=4, seed=5)
    assert set(res) == set(base) | {"f_draws", "g_draws", "h_draws"}
    assert all(_same_bits(base[k], res[k]) for k in base)
    assert all(res[k + "_draws"].shape == (4, M) for k in "fgh")
    retrieve.save_components(res, str(tmp_path / "plots"))
    for k in "fgh":
        assert _same_bits(np.load(tmp_path / "plots" / (k + "_draws.npy")), res[k + "_draws"])
    retrieve.save_components(base, str(tmp_path / "plain"))
    assert not (tmp_path / "plain" / "f_draws.npy").exists()
    with pytest.raises(ValueError):
        retrieve.retrieve_components("ST3", _chunk2d(s), pars, n_draws=4)
    # covariance.predict_draws is the handle call
    pred = [res["lwl_predict"]] * 3
    mu, Sigma, draws = covariance.predict_draws(res["lwls"], s.fl, s.sigma, pred, [0.0] * 3, syn.GP_BASE[3], 4, 5)
    assert _same_bits(mu, res["mu"]) and _same_bits(Sigma, res["Sigma"])
    assert _same_bits(draws, np.hstack([res[k + "_draws"] for k in "fgh"]))
    from psoap_amd.chunk import ChunkHandle
    with ChunkHandle(s.fl, s.sigma) as h:
        h.predict(0, res["lwls"], np.stack(pred), [0.0] * 3, list(syn.GP_BASE[3]))
        assert _same_bits(draws, h.predict_draw(4, seed=5))
    # under a baseline the marginal posterior is the one drawn from
    marg = retrieve.retrieve_components("ST3", _chunk2d(s), pars, baseline={"order": 1, "sd": [0.05, 0.02]}, n_draws=2, seed=5)
    plain = retrieve.retrieve_components("ST3", _chunk2d(s), pars, baseline={"order": 1, "sd": [0.05, 0.02]})
    assert _same_bits(marg["mu"], plain["mu"]) and _same_bits(marg["Sigma"], plain["Sigma"])
    assert marg["g_draws"].shape == (2, M) and not np.any(marg["f_draws"] == res["f_draws"][:2])
