"""GPU parity: vb_lse_combine and vb_lse_combine_strided against bsa_oracle.combine_reference, bf16 and
fp16, D = 64 and 128, with alpha requested, on rows dealt into the classes where the combine's arithmetic
has an edge: alpha near 1/2, the smaller exponential an fp16 subnormal, the exponentials underflowing,
LSEs near 250 (their own storage rounding moves the weights), and the -inf LSEs of an absent branch.

Cases, bounds and checks are tests/combine_cases.py's (its docstring derives (a) to (d) from the
arithmetic); tests/test_lse_combine_ref.py holds the cases and the bounds to the reference alone, on the
CPU, and shows that the checks fail for b = a, for an unrounded e1 and for flushed fp16 subnormals.
The strided entry is compared with the reference as well, not only with the contiguous entry: an error
in the arithmetic the two kernels share cancels out of that comparison (tests/test_gpu_io_layout.py)."""
import pytest
import torch

import combine_cases as C
from combine_cases import CASES, IDS, make_case

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()


@pytest.mark.parametrize("entry", ["contiguous", "strided"])
@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_combine_matches_the_reference(idx, entry):
    from vblade import ops
    c = make_case(idx)
    B, H, L, D = c.shape
    out1, out2 = c.out1.to(DEV), c.out2.to(DEV)
    kw = {}
    if entry == "strided":
        # out1 and the output in [B,L,H,D] memory, out2 contiguous: every stride set of the strided kernel
        out1 = out1.transpose(1, 2).contiguous().transpose(1, 2)
        kw = dict(out_layout="blhd")
    out, alpha = ops.lse_combine(out1, c.lse1.to(DEV), out2, c.lse2.to(DEV), c.gap, **kw)
    assert tuple(out.shape) == (B, H, L, D) and out.dtype == c.dtype
    assert tuple(alpha.shape) == (B, H, L) and alpha.dtype == torch.float32
    if entry == "strided":
        assert out.transpose(1, 2).is_contiguous()
    C.assert_combine(c, out.cpu(), alpha.cpu())
