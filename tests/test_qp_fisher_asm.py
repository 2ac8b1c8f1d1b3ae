"""CPU (needs hipcc, no GPU): the device assembly of the two kernels of psoap_chunk_fisher_qp, on the library as built from the
sources in the tree (psoap_amd/asmcheck.py, as tests/test_hot_loops.py uses it).

k_qp_fisher_contract<C> has two K loops in front of the heaviest epilogue in the library: whatever the epilogue holds too long
the register allocator takes out of the loops' operand registers, as scratch traffic in every turn (profiles/quasiperiodic.md).
No instance C = 1, 2, 3 may have a scratch instruction between its first and its last MFMA, or ahead of the first; spills behind
the last MFMA are paid once per tile and are reported (profiles/quasiperiodic_fisher.md).  k_qp_fisher_tangent_fill<C> has no
MFMA and no accumulator tile: it spills no vector register at all."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _have_hipcc():
    from psoap_amd import build
    return shutil.which(build.hipcc()) is not None


pytestmark = pytest.mark.skipif(not _have_hipcc(), reason="needs hipcc")


def test_no_scratch_in_or_ahead_of_the_mfma_loops_of_the_contraction():
    from psoap_amd import asmcheck, build
    res = asmcheck.scan_mfma_scratch(build.device_asm(), "k_qp_fisher_contract")
    assert len(res) == 3, sorted(res)
    for name, (mfma, ahead, inside, behind) in sorted(res.items()):
        print(f"{name}: {mfma} MFMAs, scratch instructions ahead {ahead}, inside {inside}, behind {behind}")
        assert mfma >= 2 * 64, (name, mfma)          # two K loops of at least one 64-MFMA stage each
        assert ahead == 0 and inside == 0, (name, ahead, inside)


def test_the_gradient_kernel_the_epilogue_is_shared_with_keeps_its_loops_clean():
    from psoap_amd import asmcheck, build
    res = asmcheck.scan_mfma_scratch(build.device_asm(), "k_qp_grad_contract")
    assert len(res) == 3, sorted(res)
    assert all(v[1] == 0 and v[2] == 0 for v in res.values()), res


def test_the_tangent_fill_has_no_mfma_and_spills_no_vector_register():
    from psoap_amd import asmcheck, build
    text = build.device_asm()
    scan = asmcheck.scan_mfma_scratch(text, "k_qp_fisher_tangent_fill")
    assert len(scan) == 3 and all(v == (0, 0, 0, 0) for v in scan.values()), scan
    res = {k: v for k, v in asmcheck.kernel_resources(text).items() if "k_qp_fisher_" in k}
    assert len(res) == 7, sorted(res)                # three fills, three contractions, the dot
    for k, v in sorted(res.items()):
        print(k, v)
        if "tangent_fill" in k or "fisher_dot" in k:
            assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
