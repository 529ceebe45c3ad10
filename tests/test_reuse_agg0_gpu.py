"""GPU side of ``reuse_agg0``: the executor with and without the reused layer-0 aggregate,
bitwise over three training steps on the device kernels, and the property the reuse rests
on — ``gemm_f32`` with its second operand aliasing the left columns of its own output rows
(csrc/kernels/gemm_f32.hip, "In place") equals the same GEMM with a separate operand."""
import pytest
import torch

from dgraph_amd.ops import f32 as F32
from test_reuse_agg0 import _assert_same_steps, _executor, _train  # tests/ is on sys.path

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("hidden,feat", [(256, None), (128, 100)])
def test_reuse_agg0_bitwise_gpu(hidden, feat):
    res = {}
    for reuse in ("auto", "off"):
        ex, model, g = _executor(0, 1, reuse, dev=DEV, hidden=hidden, feat=feat)
        assert ex.schedule["reuse_agg0"] is (reuse == "auto")
        assert len(ex.chunks) > 1
        res[reuse] = _train(ex, model, g)
        nnz = ex.nnz_it + ex.nnz_h
    _assert_same_steps(res["auto"], res["off"])
    assert res["auto"][1][3] == res["off"][1][3] - nnz
    assert res["auto"][0][3] == res["off"][0][3]


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("M", [1, 255, 257, 773, "2x256xCUs+5"])
@pytest.mark.parametrize("K2,N", [(128, 256), (128, 128)])
def test_gemm_f32_second_operand_in_output_rows(K2, N, M):
    """out = relu([A1 | A2] [B1; B2] + bias) with A2 = out[:, :K2] (row stride N), as the
    forward of layer 0 runs it: every block takes its A rows through all K stages before it
    stores the tile; the largest M gives every block more than one (dynamically pulled)
    tile, so the next tile's prefetch runs over the current tile's stores."""
    if isinstance(M, str):
        M = 2 * 256 * _cus() + 5
    K1 = 128
    g = torch.Generator().manual_seed(M % 1000 + N)
    A1 = torch.randn(M, K1, generator=g).to(DEV)
    A2 = torch.randn(M, K2, generator=g).to(DEV)
    B1 = (torch.randn(K1, N, generator=g) / 8).to(DEV)
    B2 = (torch.randn(K2, N, generator=g) / 8).to(DEV)
    bias = torch.randn(N, generator=g).to(DEV)
    sep = torch.empty(M, N, device=DEV)
    F32.gemm_f32(A1, B1, A2, B2, bias=bias, relu=True, out=sep)
    buf = torch.full((M, N), float("nan"), device=DEV)
    buf[:, :K2] = A2
    view = buf[:, :K2]
    assert view.stride(0) == N and view.data_ptr() == buf.data_ptr()
    F32.gemm_f32(A1, B1, view, B2, bias=bias, relu=True, out=buf)
    assert torch.equal(buf, sep)
    # and against fp64 on a sample of rows (the whole product at the small sizes)
    rows = torch.arange(M) if M <= 1024 else torch.randint(0, M, (1024,), generator=g)
    rows = rows.to(DEV)
    ref = (A1[rows].double() @ B1.double() + A2[rows].double() @ B2.double()
           + bias.double()).clamp_min(0)
    torch.testing.assert_close(sep[rows].double(), ref, atol=1e-4, rtol=1e-5)
