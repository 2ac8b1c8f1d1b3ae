"""Component-spectrum reconstruction of one chunk: the body of the reference's retrieve scripts
(/root/reference/scripts/psoap_retrieve_SB2.py:40-160, psoap_retrieve_ST3.py:40-170) without the plotting.

``retrieve_components`` evaluates the orbit at the chunk's dates, shifts the ln-wavelengths to every
component's rest frame, masks, predicts all components on a grid twice as fine as the data spanning the
primary's rest-frame range (``n_pix_predict = 2 n_pix``, SB2:96-105 / ST3:97-109) with prior means 0, and
splits ``mu`` / ``sqrt(diag(Sigma))`` per component.  Orbit solve and the conditional run on the device.
``save_components`` writes what the scripts write: ``f.npy``, ``g.npy`` (, ``h.npy``) as
``vstack((wl_predict, mu_k, sigma_k))``, ``mu.npy`` and ``Sigma.npy`` (SB2:150-155), and with draws
``f_draws.npy``, ``g_draws.npy`` (, ``h_draws.npy``), each ``(n_draws, M)`` (psoap_retrieve_ST3_draw.py:51-68).
"""
from __future__ import annotations

import os

import numpy as np

from . import covariance, orbit
from .data import c_kms, epoch_index_of
from .utils import N_COMPONENTS, n_params_orb, registered_params

_NAMES = "fgh"


def retrieve_components(model, chunk, parameters, n_pix_predict=None, get_Sigma=True, baseline=None, n_draws=0, seed=None,
                        nugget=1e-8):
    """``chunk``: an UNMASKED ``psoap_amd.data.Chunk`` (2-D arrays); ``parameters``: the config's
    ``parameters`` dictionary (every registered parameter of ``model``).  Returns a dict with
    ``wl_predict``, ``lwl_predict``, ``mu`` (c * M,), ``Sigma`` (c * M, c * M) or None, and per
    component ``mu_f`` / ``sigma_f`` (, ``_g``, ``_h``).

    ``baseline``: the dictionary ``ChunkWorker(baseline=...)`` takes -- ``order``, ``sd`` (order + 1 prior standard
    deviations) and optionally ``weight`` (``"flux"``: the polynomial multiplies the flux; ``"one"``: additive).  With it the
    prediction conditions under the per-epoch continuum polynomial integrated out (``covariance.predict_marginal``), so
    ``sigma_f`` / ``sigma_g`` / ``sigma_h`` carry the continuum's uncertainty, as the orbit and hyper-parameter error bars of
    a fit under that baseline do.

    ``n_draws > 0``: the result also carries ``f_draws`` / ``g_draws`` (/ ``h_draws``), each ``(n_draws, M)``: spectra drawn
    on the device from ``N(mu, Sigma + nugget I)`` (``covariance.predict_draws``; the reference's ``_draw`` scripts call
    ``np.random.multivariate_normal(mu, Sigma)`` on the host) with the generator's ``seed`` (required).  They show which
    line depths and blends the data pin down, which the diagonal ``sigma_f`` cannot.  ``get_Sigma`` then only decides what
    is returned.  With ``n_draws == 0`` nothing changes."""
    if model not in ("SB2", "ST3", "SB1"):
        raise ValueError("retrieve_components supports SB1, SB2 and ST3 (the models the reference has scripts for)")
    c = N_COMPONENTS[model]
    reg = registered_params[model]
    p_orb = [parameters[n] for n in reg[:n_params_orb[model]]]
    p_gp = [parameters[n] for n in reg[n_params_orb[model]:]]
    mask = np.asarray(chunk.mask, dtype=bool)
    lwl2d = np.log(np.asarray(chunk.wl, dtype=np.float64)) if np.ndim(chunk.wl) == 2 else None
    if lwl2d is None:
        raise ValueError("retrieve_components needs the 2-D chunk: call it before apply_mask()")
    vel = np.atleast_2d(orbit.models[model](*p_orb, np.asarray(chunk.date1D)).get_velocities())   # (c, n_epochs)
    ep = epoch_index_of(mask)
    lwl = lwl2d[mask]
    lwls = lwl[None, :] + (-vel[:, ep]) / c_kms          # lredshift(lwls, -v) per epoch (data.py:37)
    fl = np.asarray(chunk.fl, dtype=np.float64)[mask]
    sigma = np.asarray(chunk.sigma, dtype=np.float64)[mask]
    M = int(n_pix_predict) if n_pix_predict is not None else 2 * int(chunk.n_pix)
    lwl_predict = np.linspace(np.min(lwls[0]), np.max(lwls[0]), num=M)
    pred = [lwl_predict] * c
    if int(n_draws) > 0:
        return _retrieve_draws(c, lwls, fl, sigma, lwl, ep, lwl_predict, p_gp, get_Sigma, baseline, int(n_draws), seed, nugget)
    if baseline is not None:
        return _retrieve_marginal(c, lwls, fl, sigma, lwl, ep, lwl_predict, p_gp, get_Sigma, baseline)
    if isinstance(get_Sigma, str):
        # get_Sigma="diag": the per-component means and standard deviations only -- what the scripts plot and save as
        # f.npy / g.npy / h.npy -- without the (c M)^2 covariance matrix (psoap_predictor_run_var)
        if get_Sigma != "diag":
            raise ValueError('get_Sigma must be True, False or "diag"')
        mu, var = covariance.predict_components_var(lwls, fl, sigma, pred, [0.0] * c, p_gp)
        out = {"wl_predict": np.exp(lwl_predict), "lwl_predict": lwl_predict, "mu": mu, "Sigma": None, "lwls": lwls}
        sd = np.sqrt(var)
        for k in range(c):
            out["mu_" + _NAMES[k]] = mu[k * M:(k + 1) * M]
            out["sigma_" + _NAMES[k]] = sd[k * M:(k + 1) * M]
        return out
    if c == 1:
        res = covariance.predict_f(lwls[0], fl, sigma, lwl_predict, *p_gp, mu_GP=0.0)
        mu, Sigma = res
    elif c == 2:
        res = covariance.predict_f_g(lwls[0], lwls[1], fl, sigma, pred[0], pred[1], 0.0, p_gp[0], p_gp[1], 0.0,
                                     p_gp[2], p_gp[3], get_Sigma=get_Sigma)
        mu, Sigma = res if get_Sigma else (res, None)
    else:
        mu, Sigma = covariance.predict_f_g_h(lwls[0], lwls[1], lwls[2], fl, sigma, *pred, 0.0, 0.0, 0.0, *p_gp)
    out = {"wl_predict": np.exp(lwl_predict), "lwl_predict": lwl_predict, "mu": mu, "Sigma": Sigma, "lwls": lwls}
    sd = np.sqrt(np.diag(Sigma)) if Sigma is not None else None
    for k in range(c):
        out["mu_" + _NAMES[k]] = mu[k * M:(k + 1) * M]
        if sd is not None:
            out["sigma_" + _NAMES[k]] = sd[k * M:(k + 1) * M]
    return out


def _retrieve_marginal(c, lwls, fl, sigma, lwl, ep, lwl_predict, p_gp, get_Sigma, baseline):
    """the prediction of ``retrieve_components`` under ``baseline``: ``x`` is the observed-frame ln-wavelengths of the unmasked
    pixels, the epoch index that of the mask"""
    unknown = set(baseline) - {"order", "sd", "weight"}
    if unknown or not {"order", "sd"} <= set(baseline):
        raise ValueError(f"baseline needs 'order' and 'sd' (and optionally 'weight'); got {sorted(baseline)}")
    kind = baseline.get("weight", "one")
    if kind not in ("one", "flux"):
        raise ValueError("baseline['weight'] must be 'one' or 'flux'")
    weight = fl if kind == "flux" else None
    if isinstance(get_Sigma, str) and get_Sigma != "diag":
        raise ValueError('get_Sigma must be True, False or "diag"')
    M = lwl_predict.shape[0]
    want = get_Sigma if isinstance(get_Sigma, str) else bool(get_Sigma)
    res = covariance.predict_marginal(lwls, fl, sigma, [lwl_predict] * c, [0.0] * c, p_gp, lwl, ep, int(baseline["order"]),
                                      baseline["sd"], weight, mode=2 if c == 1 else 0, want_sigma=want)
    mu, second = res if want else (res, None)
    Sigma = second if want is True else None
    out = {"wl_predict": np.exp(lwl_predict), "lwl_predict": lwl_predict, "mu": mu, "Sigma": Sigma, "lwls": lwls}
    sd = None if second is None else np.sqrt(second if want == "diag" else np.diag(second))
    for k in range(c):
        out["mu_" + _NAMES[k]] = mu[k * M:(k + 1) * M]
        if sd is not None:
            out["sigma_" + _NAMES[k]] = sd[k * M:(k + 1) * M]
    return out


def _baseline_weight(baseline, fl):
    unknown = set(baseline) - {"order", "sd", "weight"}
    if unknown or not {"order", "sd"} <= set(baseline):
        raise ValueError(f"baseline needs 'order' and 'sd' (and optionally 'weight'); got {sorted(baseline)}")
    kind = baseline.get("weight", "one")
    if kind not in ("one", "flux"):
        raise ValueError("baseline['weight'] must be 'one' or 'flux'")
    return fl if kind == "flux" else None


def _retrieve_draws(c, lwls, fl, sigma, lwl, ep, lwl_predict, p_gp, get_Sigma, baseline, n_draws, seed, nugget):
    """``retrieve_components`` with ``n_draws > 0``: the posterior (plain, or under ``baseline``) through the chunk's cached
    handle, and the draws from it split per component"""
    if seed is None:
        raise ValueError("retrieve_components(n_draws > 0) needs a seed")
    if isinstance(get_Sigma, str) and get_Sigma != "diag":
        raise ValueError('get_Sigma must be True, False or "diag"')
    marg = None
    if baseline is not None:
        marg = {"x": lwl, "epoch_index": ep, "order": int(baseline["order"]), "prior_sd": baseline["sd"],
                "weight": _baseline_weight(baseline, fl)}
    M = lwl_predict.shape[0]
    mu, Sigma, draws = covariance.predict_draws(lwls, fl, sigma, [lwl_predict] * c, [0.0] * c, p_gp, n_draws, seed,
                                                mode=2 if c == 1 else 0, nugget=nugget, baseline=marg)
    out = {"wl_predict": np.exp(lwl_predict), "lwl_predict": lwl_predict, "mu": mu, "Sigma": Sigma if get_Sigma is True else None,
           "lwls": lwls}
    sd = np.sqrt(np.diag(Sigma)) if get_Sigma else None
    for k in range(c):
        out["mu_" + _NAMES[k]] = mu[k * M:(k + 1) * M]
        if sd is not None:
            out["sigma_" + _NAMES[k]] = sd[k * M:(k + 1) * M]
        out[_NAMES[k] + "_draws"] = np.ascontiguousarray(draws[:, k * M:(k + 1) * M])
    return out


def retrieve_components_at(model, chunk, parameters, tau, dates, n_pix_predict=None, get_Sigma="diag", n_draws=0, seed=None,
                           nugget=1e-8):
    """``retrieve_components`` under time-variable component spectra (``covariance.predict_timevar``): the spectrum of every
    component at each of ``dates`` (in the unit and from the origin of ``chunk.date1D``), for time scales ``tau`` (c,) -- ``inf``
    keeps a component static -- as ``optimize_GP_timevar`` finds them.  ONE device call over ``len(dates)`` runs of
    ``retrieve_components``' prediction grid, the date of run ``d`` being ``dates[d] - min(chunk.date1D)``.

    Returns ``wl_predict``, ``lwl_predict`` (M,), ``dates``, ``lwls``, ``mu`` (c * n_dates * M,) -- component by component, date
    by date -- and ``Sigma`` (``get_Sigma=True``: the full matrix, the covariances between dates in it; else None), and per
    component ``mu_f`` / ``sigma_f`` (, ``_g``, ``_h``) of shape ``(n_dates, M)`` (``sigma_*`` unless ``get_Sigma`` is False).
    ``n_draws > 0`` (needs ``seed``): ``f_draws`` (, ``g_``, ``h_``) of shape ``(n_draws, n_dates, M)`` from ``N(mu, Sigma +
    nugget I)``: every draw is one history of the spectrum over the dates."""
    if model not in ("SB2", "ST3", "SB1"):
        raise ValueError("retrieve_components_at supports SB1, SB2 and ST3 (the models the reference has scripts for)")
    if isinstance(get_Sigma, str) and get_Sigma != "diag":
        raise ValueError('get_Sigma must be True, False or "diag"')
    if int(n_draws) > 0 and seed is None:
        raise ValueError("retrieve_components_at(n_draws > 0) needs a seed")
    c = N_COMPONENTS[model]
    reg = registered_params[model]
    p_orb = [parameters[n] for n in reg[:n_params_orb[model]]]
    p_gp = [parameters[n] for n in reg[n_params_orb[model]:]]
    mask = np.asarray(chunk.mask, dtype=bool)
    if np.ndim(chunk.wl) != 2:
        raise ValueError("retrieve_components_at needs the 2-D chunk: call it before apply_mask()")
    lwl2d = np.log(np.asarray(chunk.wl, dtype=np.float64))
    date1D = np.asarray(chunk.date1D, dtype=np.float64)
    vel = np.atleast_2d(orbit.models[model](*p_orb, date1D).get_velocities())   # (c, n_epochs)
    ep = epoch_index_of(mask)
    lwls = lwl2d[mask][None, :] + (-vel[:, ep]) / c_kms
    fl = np.asarray(chunk.fl, dtype=np.float64)[mask]
    sigma = np.asarray(chunk.sigma, dtype=np.float64)[mask]
    M = int(n_pix_predict) if n_pix_predict is not None else 2 * int(chunk.n_pix)
    lwl_predict = np.linspace(np.min(lwls[0]), np.max(lwls[0]), num=M)
    dates = np.atleast_1d(np.asarray(dates, dtype=np.float64))
    D = dates.shape[0]
    t0 = date1D.min()
    times = date1D[ep] - t0
    t_predict = np.repeat(dates - t0, M)
    pred = [np.tile(lwl_predict, D)] * c
    mode = 2 if c == 1 else 0
    draws = None
    if int(n_draws) > 0:
        mu, second, draws = covariance.predict_draws(lwls, fl, sigma, pred, [0.0] * c, p_gp, int(n_draws), seed, mode=mode, nugget=nugget,
                                                     timevar={"times": times, "tau": tau, "t_predict": t_predict})
        want = True
    else:
        want = get_Sigma if isinstance(get_Sigma, str) else bool(get_Sigma)
        res = covariance.predict_timevar(lwls, fl, sigma, pred, t_predict, [0.0] * c, p_gp, tau, times, mode=mode, want_sigma=want)
        mu, second = res if want else (res, None)
    out = {"wl_predict": np.exp(lwl_predict), "lwl_predict": lwl_predict, "dates": dates, "mu": mu,
           "Sigma": second if (want is True and get_Sigma is True) else None, "lwls": lwls}
    sd = None
    if second is not None and get_Sigma:
        sd = np.sqrt(second if want == "diag" else np.diag(second))
    for k in range(c):
        sl = slice(k * D * M, (k + 1) * D * M)
        out["mu_" + _NAMES[k]] = mu[sl].reshape(D, M)
        if sd is not None:
            out["sigma_" + _NAMES[k]] = sd[sl].reshape(D, M)
        if draws is not None:
            out[_NAMES[k] + "_draws"] = np.ascontiguousarray(draws[:, sl]).reshape(int(n_draws), D, M)
    return out


def retrieve_posterior(model, chunk, parameters, flatchain, fix_params, n_samples=64, thin_seed=0, n_pix_predict=None,
                       get_Sigma=True, baseline=None, draws_per_sample=0, seed=None):
    """``retrieve_components`` marginalised over the chain instead of taken at one parameter vector: the component spectra
    under the posterior of the orbit and the hyper-parameters, by the law of total covariance over chain samples
    (``covariance.predict_mixture``: every sample is predicted and folded on the device).

    ``flatchain`` ``(n, n_free)``: rows in the layout ``utils.convert_vector`` takes, the parameters named in ``fix_params``
    held at their values in ``parameters``.  ``n_samples`` rows are picked without replacement by
    ``numpy.random.default_rng(thin_seed)`` (all rows when there are fewer) and weigh the same.  The orbits of all of them
    are evaluated in one batched device call.

    Every sample is predicted on ONE grid: ``retrieve_components``' own, taken at ``parameters`` -- ``linspace(min, max)``
    of the primary's rest-frame range at the point estimate.  A per-sample grid would make the means incomparable: the
    between-sample term is the scatter of ``mu_s`` at fixed rest wavelengths.

    Returns the dict ``retrieve_components`` returns (``save_components`` works on it unchanged; ``lwls`` are the grids at
    ``parameters``), where ``sigma_f`` (, ``_g``, ``_h``) now carry the orbit's and the hyper-parameters' uncertainty, and
    beside it ``sigma_within_f`` / ``sigma_between_f`` (, ``_g``, ``_h``) -- the square roots of the two terms' diagonals,
    ``sigma_f**2 = sigma_within_f**2 + sigma_between_f**2`` --, ``n_folded`` and ``skipped`` (positions among the picked
    rows whose data covariance was not positive definite), and ``rows``, the picked chain rows.  ``get_Sigma`` other than
    True accumulates variances only and ``Sigma`` is None.  With one sample equal to ``parameters`` the result is
    ``retrieve_components``'.  ``baseline``: as ``retrieve_components``.  ``draws_per_sample > 0`` (needs ``seed`` and
    ``get_Sigma=True``): ``f_draws`` (, ``g_``, ``h_``), ``(n_folded * draws_per_sample, M)`` each -- draws from the
    mixture, sample ``s`` with the generator's seed ``seed + s``."""
    from .utils import convert_vectors
    if model not in ("SB2", "ST3", "SB1"):
        raise ValueError("retrieve_posterior supports SB1, SB2 and ST3 (the models the reference has scripts for)")
    if isinstance(get_Sigma, str) and get_Sigma != "diag":
        raise ValueError('get_Sigma must be True, False or "diag"')
    c = N_COMPONENTS[model]
    reg = registered_params[model]
    chain = np.atleast_2d(np.asarray(flatchain, dtype=np.float64))
    n = chain.shape[0]
    rows = np.arange(n) if n <= int(n_samples) else np.sort(np.random.default_rng(thin_seed).choice(n, size=int(n_samples), replace=False))
    p_orb, p_gp = convert_vectors(chain[rows], model, fix_params, **{k: parameters[k] for k in fix_params})
    mask = np.asarray(chunk.mask, dtype=bool)
    if np.ndim(chunk.wl) != 2:
        raise ValueError("retrieve_posterior needs the 2-D chunk: call it before apply_mask()")
    lwl2d = np.log(np.asarray(chunk.wl, dtype=np.float64))
    # the point estimate rides along as the last orbit of the batch: its primary fixes the grid
    p0 = np.array([[parameters[k] for k in reg[:n_params_orb[model]]]], dtype=np.float64)
    vel = orbit.velocities(model, np.concatenate([p_orb, p0]), np.asarray(chunk.date1D))      # (S + 1, c, n_epochs)
    ep = epoch_index_of(mask)
    lwl = lwl2d[mask]
    lwls_all = lwl[None, None, :] + (-vel[:, :, ep]) / c_kms
    lwls0 = lwls_all[-1]
    fl = np.asarray(chunk.fl, dtype=np.float64)[mask]
    sigma = np.asarray(chunk.sigma, dtype=np.float64)[mask]
    M = int(n_pix_predict) if n_pix_predict is not None else 2 * int(chunk.n_pix)
    lwl_predict = np.linspace(np.min(lwls0[0]), np.max(lwls0[0]), num=M)
    marg = None
    if baseline is not None:
        marg = {"x": lwl, "epoch_index": ep, "order": int(baseline["order"]), "prior_sd": baseline["sd"],
                "weight": _baseline_weight(baseline, fl)}
    full = get_Sigma is True
    res = covariance.predict_mixture(lwls_all[:-1], fl, sigma, [lwl_predict] * c, [0.0] * c, p_gp, mode=2 if c == 1 else 0,
                                     baseline=marg, want_sigma=full, draws_per_sample=draws_per_sample, seed=seed)
    mu, Sigma = res["mu"], res["Sigma"]
    out = {"wl_predict": np.exp(lwl_predict), "lwl_predict": lwl_predict, "mu": mu, "Sigma": Sigma, "lwls": lwls0,
           "n_folded": res["n_folded"], "skipped": res["skipped"], "rows": rows}
    sd = np.sqrt(np.diag(Sigma)) if full else np.sqrt(res["var_within"] + res["var_between"])
    sd_w, sd_b = np.sqrt(res["var_within"]), np.sqrt(res["var_between"])
    for k in range(c):
        sl = slice(k * M, (k + 1) * M)
        out["mu_" + _NAMES[k]] = mu[sl]
        out["sigma_" + _NAMES[k]] = sd[sl]
        out["sigma_within_" + _NAMES[k]] = sd_w[sl]
        out["sigma_between_" + _NAMES[k]] = sd_b[sl]
        if "draws" in res:
            out[_NAMES[k] + "_draws"] = np.ascontiguousarray(res["draws"][:, sl])
    return out


def save_components(result, outdir):
    """Write ``f.npy``, ``g.npy`` (, ``h.npy``), ``mu.npy``, ``Sigma.npy`` into ``outdir`` (the scripts'
    ``plots_chunk_*`` directory), and ``f_draws.npy``, ``g_draws.npy`` (, ``h_draws.npy``) where the result has draws."""
    os.makedirs(outdir, exist_ok=True)
    for k in _NAMES:
        if "mu_" + k in result and "sigma_" + k in result:
            np.save(os.path.join(outdir, k + ".npy"), np.vstack((result["wl_predict"], result["mu_" + k], result["sigma_" + k])))
        if k + "_draws" in result:
            np.save(os.path.join(outdir, k + "_draws.npy"), result[k + "_draws"])
    np.save(os.path.join(outdir, "mu.npy"), result["mu"])
    if result["Sigma"] is not None:
        np.save(os.path.join(outdir, "Sigma.npy"), result["Sigma"])
