"""Policy of the sign-masked pooled exchange source (parallel/factored.py ``source="pooled-masked"``) and
the torch reference of its format (parallel/pooled_masked.py).  On the CPU no layer offers a pooled input,
so a Linear under this source still sends its rows."""
import pytest
import torch

from torch_distributed_sandbox_amd.parallel import factored
from torch_distributed_sandbox_amd.parallel import pooled_masked as pm


def test_source_is_accepted_and_a_plain_linear_sends_rows():
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    assert "pooled-masked" in factored.EXCHANGE_SOURCES
    w = torch.nn.Parameter(torch.zeros(10, 32 * 64 * 64))
    ex = factored.ActivationExchange(w, None, None, 2, "activations", lambda on: None, lambda: None, None,
                                     source="pooled-masked")
    ex.arm(True)
    # a CPU weight has no fused head behind it: the activation path is planned, from the rows
    assert ex.source == "pooled-masked" and not ex.pooled_capable()
    assert ex.planned(2) == "activations" and ex.grouped(2, w.shape[1])
    ex.detach()
    assert DistributedDataParallel(torch.nn.Linear(8, 4), exchange_source="pooled-masked").exchange_source == \
        "pooled-masked"


@pytest.mark.parametrize("B,Q,cap", [(1, 9, 100), (5, 750, 45_000_000), (3, 260, 1)])
def test_reported_bytes(B, Q, cap):
    q4, q8 = -(-Q // 4), -(-Q // 8)
    pages = B * 32 * q4 * -(-q8 // 32)
    assert pm.npages(B, Q) == pages and pm.meta_numel(B, Q) == 33 * pages
    assert pm.payload_bytes(B, Q, cap) == 132 * pages + 2 * cap + 512


@pytest.mark.parametrize("B,Q", [(1, 9), (2, 11), (1, 260)])
def test_reference_round_trip(B, Q):
    """decode_ref(encode_ref(ya)) is relu(a*y + b) on the image, in the fc's flatten order; the kept count
    is the number of non-zero X."""
    q4, q8, _ = pm.geom(Q)
    g = torch.Generator().manual_seed(Q)
    ya = torch.randn(B, 32, q4 * q8 * 32, generator=g).half()
    rec = torch.zeros(128)
    rec[:32], rec[32:64] = torch.randn(32, generator=g), torch.randn(32, generator=g) * 0.3
    rec[64:67], rec[68:100] = torch.tensor([0.5, 1.0, 1.0]), torch.randn(32, generator=g) * 0.1
    meta, vals, nnz = pm.encode_ref(ya, rec, Q)
    x = pm.decode_ref(meta, vals, rec, B, Q)
    h = ya.view(B, 32, q4, q8, 4, 8).permute(0, 1, 2, 4, 3, 5).reshape(B, 32, 4 * q4, 8 * q8)[:, :, :Q, :Q].double()
    a, b, b2 = (rec[s].double().view(1, 32, 1, 1) for s in (slice(0, 32), slice(32, 64), slice(68, 100)))
    ref = torch.relu(a * (h * 0.5 + b2) + b).reshape(B, -1)
    assert x.shape == (B, 32 * Q * Q) and torch.allclose(x.double(), ref, rtol=1e-6, atol=1e-6)
    assert nnz == int((x != 0).sum()) and meta.view(-1, 33)[0, 0] == 0
