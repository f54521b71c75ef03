"""The per-(device, stream) buffers of gts._operands.StreamBuffers behind dense._gemm_ws, ops._gat_ws and
ops.cluster_counters: reuse, growth, one buffer per stream, no aliasing between uses."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _overlap(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def test_stream_buffers_reuse_grow_and_keep_uses_and_streams_apart(hip_lib):
    from gts import dense, ops
    from gts._operands import StreamBuffers

    assert torch.cuda.is_available()
    use = StreamBuffers()
    first = use.get(DEV, 1000)
    assert first.dtype == torch.float32 and first.numel() * 4 >= 1000           # rounded up to whole floats
    assert use.get(DEV, 1000) is first and use.get(DEV, 10) is first and use.get(DEV, 0) is first
    grown = use.get(DEV, 4096 + 1)
    assert grown is not first and grown.numel() * 4 >= 4097
    assert use.get(DEV, 0) is grown, "a request of 0 bytes returns the live buffer"
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        other = use.get(DEV, 1000)
        assert other is not grown and not _overlap(other, grown)
        assert use.get(DEV, 500) is other
    assert use.get(DEV, 0) is grown

    # two uses on one stream: the GEMM workspace and the GAT workspace never alias
    gemm, gat = dense._gemm_ws.get(DEV, 2048), ops._gat_ws(DEV, 2048)
    assert gemm is not gat and not _overlap(gemm, gat)
    assert ops._gat_ws(DEV, 0) is gat and dense._gemm_ws.get(DEV, 0) is gemm

    counters = ops.cluster_counters(DEV)
    assert counters.dtype == torch.int32 and counters.numel() == 256 and int(counters.abs().max()) == 0
    assert ops.cluster_counters(DEV) is counters
    assert not _overlap(counters, gemm) and not _overlap(counters, gat)
    with torch.cuda.stream(side):
        theirs = ops.cluster_counters(DEV)
        assert theirs is not counters and int(theirs.abs().max()) == 0
