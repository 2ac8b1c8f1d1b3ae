"""The row-granular clip on the device: every matrix's updates start at its own first 16-row group (DagMat::first, k_sky_fine)
and the results keep their bits -- against a handle created under PSOAP_SKY_FINE=0 (whole-panel starts) and one under
PSOAP_SKY_CLIP=0 (the union's ranges), with the stages against the host twin (tests/test_sky_fine.py)."""
import numpy as np
import pytest

from test_sky_clip import sky_clip
from test_sky_fine import GPT, sky_clip16
from test_sky_order import gpu_case

pytestmark = pytest.mark.gpu

B = 16
N = 1250


@pytest.fixture(autouse=True)
def scheme0(monkeypatch):
    monkeypatch.setenv("PSOAP_DAG_SCHEME", "0")
    for name in ("PSOAP_SKYLINE", "PSOAP_SKY_ORDER", "PSOAP_SKY_CLIP", "PSOAP_SKY_FINE"):
        monkeypatch.delenv(name, raising=False)


def evaluate(fl, sigma, lwl, gps, monkeypatch, **env):
    """lnprob and sky_stats of a fresh handle created under `env`"""
    from psoap_amd.chunk import ChunkHandle
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with ChunkHandle(fl, sigma, max_batch=B) as h:
        out = h.lnlike_batch(lwl, gps)
        st = h.sky_stats()
    for k in env:
        monkeypatch.delenv(k)
    return out, st


def run(fl, sigma, lwl, gps, monkeypatch, narrowed):
    """three handles, one result; the stages are the twin's.  narrowed: some column starts inside its first tile"""
    first_b, units, _ = sky_clip(lwl, gps)
    first16_b, stages, _ = sky_clip16(lwl, gps)
    assert (first16_b > GPT * first_b).any() == narrowed
    got, st = evaluate(fl, sigma, lwl, gps, monkeypatch)
    coarse, st_coarse = evaluate(fl, sigma, lwl, gps, monkeypatch, PSOAP_SKY_FINE="0")
    off, st_off = evaluate(fl, sigma, lwl, gps, monkeypatch, PSOAP_SKY_CLIP="0")
    print(f"units planned {st['units_planned']}, clipped {st['units_clipped']}, stages {st['stages_clipped']} "
          f"({st['stages_clipped'] / (GPT * st['units_clipped']):.4f} of 8 per unit)")
    assert np.all(np.isfinite(got))
    assert np.array_equal(got, coarse), np.max(np.abs(got - coarse))
    assert np.array_equal(got, off), np.max(np.abs(got - off))
    assert st["skyline_on"] == st_coarse["skyline_on"] == st_off["skyline_on"] == 1
    assert st["units_clipped"] == st_coarse["units_clipped"] == units
    assert st["stages_clipped"] == stages
    assert (stages < GPT * units) == narrowed
    assert st_coarse["stages_clipped"] == GPT * units
    assert st_off["units_clipped"] == st_off["units_planned"] and st_off["stages_clipped"] == GPT * st_off["units_planned"]
    return got


@pytest.mark.parametrize("n", [N, 1280])
def test_two_components_narrow_odd_walkers(monkeypatch, n):
    fl, sigma, lwl, gps = gpu_case(2, 320, N=n)
    gps[1::2, 1::2] *= 0.3
    run(fl, sigma, lwl, gps, monkeypatch, narrowed=True)


def test_three_components(monkeypatch):
    fl, sigma, lwl, gps = gpu_case(3, 308)
    first16_b, first_b = sky_clip16(lwl, gps)[0], sky_clip(lwl, gps)[0]
    run(fl, sigma, lwl, gps, monkeypatch, narrowed=bool((first16_b > GPT * first_b).any()))


def test_a_single_matrix_takes_no_skyline_list(monkeypatch, oracle):
    """B = 1 runs a latency scheme: no skyline, nothing to clip -- 8 stages per planned unit, the usual bits"""
    monkeypatch.delenv("PSOAP_DAG_SCHEME")      # (the scheme the library picks for one matrix by itself)
    fl, sigma, lwl, gps = gpu_case(2, 320)
    got, st = evaluate(fl, sigma, lwl[:1], gps[:1], monkeypatch)
    coarse, _ = evaluate(fl, sigma, lwl[:1], gps[:1], monkeypatch, PSOAP_SKY_FINE="0")
    off, _ = evaluate(fl, sigma, lwl[:1], gps[:1], monkeypatch, PSOAP_SKYLINE="0")
    assert st["skyline_on"] == 0
    assert st["stages_clipped"] == GPT * st["units_planned"] == GPT * st["units_clipped"]
    assert np.array_equal(got, coarse) and np.array_equal(got, off)
    want = oracle.lnlike(lwl[0], fl, sigma, list(gps[0]))
    assert abs(got[0] - want) <= 1e-10 * max(1.0, abs(want))


def test_wide_kernels_sit_on_the_clamp(monkeypatch):
    """length scales x 4: every column's first row group is its clamp, 8 times its first tile -- nothing beyond the
    tile-level clip, and the same bits"""
    fl, sigma, lwl, gps = gpu_case(2, 320, scale=4.0)
    first_b, first16_b = sky_clip(lwl, gps)[0], sky_clip16(lwl, gps)[0]
    assert np.array_equal(first16_b, GPT * first_b)
    run(fl, sigma, lwl, gps, monkeypatch, narrowed=False)
