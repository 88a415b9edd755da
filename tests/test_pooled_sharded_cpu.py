"""Policy of the pooled sharded exchange source (parallel/factored.py ``source="pooled-sharded"``):
shard boundaries, which layers may take it, DDP's argument and the operator's TDS_EXCHANGE_SOURCE
switch.  On the CPU no layer offers a pooled input, so the sharded path stays on the fc rows."""
import copy
import os

import pytest
import torch

from torch_distributed_sandbox_amd.parallel import factored, launch


def _exchange(weight, world, mode, source):
    return factored.ActivationExchange(weight, None, None, world, mode, lambda on: None, lambda: None, None,
                                       source=source)


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8, 32])
def test_plane_shards_cover_and_balance(world):
    shards = factored.plane_shards(world)
    assert len(shards) == world and shards[0][0] == 0 and shards[-1][1] == 32
    assert all(shards[i][1] == shards[i + 1][0] for i in range(world - 1))  # contiguous, in rank order
    sizes = [e - a for a, e in shards]
    assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1
    # the rule of column_chunks: cuts at round(i * planes / world)
    assert [a for a, _ in shards] == [round(i * 32 / world) for i in range(world)]
    assert shards == factored.plane_shards(world, planes=32)


@pytest.mark.parametrize("groups", range(1, 41))
@pytest.mark.parametrize("per", [361, 4225, 4096])
def test_column_groups_are_ranges_the_head_launch_takes(groups, per):
    """The grouped activation exchange's column groups of 32 planes of ``per`` columns (pooled edges
    19, 65 and 64): contiguous, non-empty, covering; the head's range launch (head_pb.hip
    tds_head_fwd_pb) takes [c0, c1) only when c0 * per and (c1 - c0) * per are multiples of 4, so odd
    planes are cut at multiples of 4 channels; planes that are a multiple of 4 keep the plain
    round(i * 32 / n) cuts."""
    in_f = 32 * per
    ex = factored.ActivationExchange(torch.nn.Parameter(torch.zeros(1, 1)), None, None, 2, "activations",
                                     lambda on: None, lambda: None, None, groups=groups, source="rows")
    got = ex.column_groups(in_f, planes=32)
    assert got[0][0] == 0 and got[-1][1] == in_f
    assert all(got[i][1] == got[i + 1][0] for i in range(len(got) - 1))
    assert all(k1 > k0 for k0, k1 in got)
    assert all(k0 % per == 0 and k1 % per == 0 for k0, k1 in got)  # whole planes
    for k0, k1 in got:  # the launch's own rule
        assert k0 % 4 == 0 and (k1 - k0) % 4 == 0, (k0, k1)
    if per % 4:
        assert all(k0 % (4 * per) == 0 and (k1 - k0) % (4 * per) == 0 for k0, k1 in got)
        assert len(got) == min(groups, 8)
    else:
        n = min(groups, 32)
        cuts = [round(i * 32 / n) for i in range(n + 1)]
        assert got == [(cuts[i] * per, cuts[i + 1] * per) for i in range(n) if cuts[i + 1] > cuts[i]]
    if groups in (1, 2, 4, 8):  # these never needed another cut: the same groups at every plane size
        assert [(k0 // per, k1 // per) for k0, k1 in got] == [(i * 32 // groups, (i + 1) * 32 // groups)
                                                              for i in range(groups)]
    # column_chunks (the head backward takes any range) keeps the plain cuts
    ex.chunks = groups
    n = min(groups, 32)
    cuts = [round(i * 32 / n) for i in range(n + 1)]
    assert ex.column_chunks(in_f, planes=32) == [(cuts[i] * per, cuts[i + 1] * per) for i in range(n)
                                                 if cuts[i + 1] > cuts[i]]


def test_source_values_and_cpu_weight():
    w = torch.nn.Parameter(torch.zeros(10, 32 * 64 * 64))
    ex = _exchange(w, 2, "sharded", "pooled-sharded")
    assert ex.source == "pooled-sharded"
    # a CPU weight has no fused head behind it: neither priced nor run from the pooled input
    assert not ex.pooled_capable()
    ex.arm(True)
    assert ex.planned(2) == "sharded" and not ex.pooled(2)
    ex.detach()
    with pytest.raises(ValueError):
        _exchange(w, 2, "sharded", "pooled-shard")


def _w_ddp(rank, world, port):
    from torch_distributed_sandbox_amd.models import ConvNet
    from torch_distributed_sandbox_amd.ops import SGD, CrossEntropyLoss
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel
    from torch_distributed_sandbox_amd.parallel import distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    H, B = 232, 2  # fc.weight 10 x 107648: an exchange candidate
    torch.manual_seed(0)
    m_ex = ConvNet(image_shape=(H, H))
    m_ar = copy.deepcopy(m_ex)
    d_ex = DistributedDataParallel(m_ex, grad_exchange="sharded", exchange_source="pooled-sharded")
    d_ar = DistributedDataParallel(m_ar, grad_exchange="allreduce")
    assert d_ex.exchanges[0].source == "pooled-sharded" and not d_ex.exchanges[0].pooled_capable()
    o_ex = d_ex.attach_optimizer(SGD(m_ex.parameters(), 0.05))
    d_ar.attach_optimizer(SGD(m_ar.parameters(), 0.05))
    crit = CrossEntropyLoss()
    g = torch.Generator().manual_seed(11)
    xs = torch.rand(world, B, 1, H, H, generator=g)
    ys = torch.randint(0, 10, (world, B), generator=g)
    for d in (d_ex, d_ar):
        d.zero_grad()
        crit(d(xs[rank]), ys[rank]).backward()
    for (n, p), q in zip(m_ex.named_parameters(), m_ar.parameters()):
        if n.endswith("0.bias"):  # conv bias before BN: analytically zero, rounding noise both ways
            continue
        rel = ((p.grad - q.grad).norm() / q.grad.norm().clamp_min(1e-30)).item()
        assert rel < 1e-5, (n, rel)
    o_ex.step()
    assert d_ex.fc_grad_path() == "sharded-exchange(zs)"  # the rows path, as before
    dist.destroy_process_group()


def test_cpu_ddp_step_stays_on_rows_path():
    launch.spawn(_w_ddp, args=(2, launch.find_free_port()), nprocs=2, timeout=300)


def test_env_overrides_ddp_argument(monkeypatch):
    from torch_distributed_sandbox_amd.parallel import DistributedDataParallel

    lin = torch.nn.Linear(8, 4)
    assert DistributedDataParallel(lin).exchange_source == "pooled"
    assert DistributedDataParallel(lin, exchange_source="pooled-sharded").exchange_source == "pooled-sharded"
    monkeypatch.setenv("TDS_EXCHANGE_SOURCE", "pooled-sharded")
    assert DistributedDataParallel(lin, exchange_source="rows").exchange_source == "pooled-sharded"
    monkeypatch.setenv("TDS_EXCHANGE_SOURCE", "")  # empty: the argument stands
    assert DistributedDataParallel(lin, exchange_source="rows").exchange_source == "rows"
    monkeypatch.setenv("TDS_EXCHANGE_SOURCE", "planes")
    with pytest.raises(ValueError):
        DistributedDataParallel(lin)
    monkeypatch.delenv("TDS_EXCHANGE_SOURCE")
    with pytest.raises(ValueError):
        DistributedDataParallel(lin, exchange_source="planes")
