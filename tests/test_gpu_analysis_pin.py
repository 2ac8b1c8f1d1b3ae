"""The analysis paths behind the C ABI against their exact pin (tests/golden/analysis_pin_v1.npz, predict_pin_v1.npz and
predict_marg_pin_v1.npz, written by tests/golden/make_analysis_pin.py on an MI355X): every output bit for bit, and the per-class ``launches``, ``flops`` and
``bytes`` of ``ChunkHandle.timings()`` -- host-computed integers held in doubles -- with ``==``.  ``ms`` and ``total_ms`` are
measurements and are not compared.

The long-double tests of these paths (test_gpu_grad.py, test_gpu_orbit_grad.py, test_gpu_fisher.py, test_gpu_loo.py,
test_gpu_marg.py, test_gpu_marg_grad.py) say that the numbers are right; this one says that a change to the host layer that
should move nothing -- not a launch, not a booked flop -- moved nothing.  A change that is MEANT to move the bits or the
bookkeeping regenerates the fixture and says so.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_analysis_pin as pin  # noqa: E402

from psoap_amd._lib import K_NAMES  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fixture():
    return pin.load_pin()


def test_the_fixture_holds_exactly_the_calls():
    names = {k.rsplit("/", 1)[0] for k in _fixture() if "/" in k}
    assert names == set(pin.CALLS)


@pytest.mark.parametrize("name", list(pin.CALLS))
def test_bits_and_bookkeeping(name):
    want = {k.rsplit("/", 1)[1]: v for k, v in _fixture().items() if k.rsplit("/", 1)[0] == name}
    (got, book), = pin.run(name)
    assert set(got) | {"book"} == set(want)
    for k, v in got.items():
        differ = int(np.count_nonzero(v != want[k])) if v.shape == want[k].shape else -1
        print(f"{name}/{k}: shape {list(v.shape)}, {differ} of {v.size} words differ")
        assert v.shape == want[k].shape and differ == 0, (name, k, differ)
    for f, row, ref in zip(pin.BOOK_FIELDS, book, want["book"]):
        print(f"{name}/{f}: " + ", ".join(f"{n} {a:.17g}" for n, a in zip(K_NAMES, row)))
        assert np.array_equal(row, ref), (name, f, dict(zip(K_NAMES, zip(row, ref))))
