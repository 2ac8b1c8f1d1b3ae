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
