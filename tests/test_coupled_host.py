"""No GPU: the record exchange of the batch-coupled terms (parallel.all_gather_records) on two gloo ranks with CPU tensors, and the refusals of
batch_scope and of a gathered batch whose tie counts a float cannot hold."""
import os
import socket
import struct

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import tfc_gan_amd as T
from tfc_gan_amd import ops, parallel


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def record(rank):
    """a mask record as the kernels leave it: four 64-bit words; here a double whose low mantissa bits matter and a count beyond 2^53"""
    return torch.tensor(list(struct.unpack("<4q", struct.pack("<dqdq", 0.1 + rank * 2.0 ** -50, (1 << 60) + 3 + rank, -0.0, -1 - rank))), dtype=torch.int64)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    assert parallel.collectives_active()
    recs = parallel.all_gather_records(record(rank))
    kl = parallel.all_gather_records(torch.full((3, 5, 2), float(rank + 1)) * torch.tensor([1.0, float("inf")]))
    torch.save({"recs": recs, "kl": kl}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_all_gather_records_two_gloo_ranks_raw_bytes_in_rank_order(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [torch.load(str(tmp_path / f"r{r}.pt"), weights_only=True) for r in range(world)]
    want = torch.stack([record(r) for r in range(world)])
    for g in got:                                                   # the same on every rank, rank order, every bit
        assert g["recs"].dtype == torch.int64 and tuple(g["recs"].shape) == (world, 4)
        assert torch.equal(g["recs"], want)
        for r in range(world):
            d0, c0, d1, c1 = struct.unpack("<dqdq", struct.pack("<4q", *g["recs"][r].tolist()))
            assert d0 == 0.1 + r * 2.0 ** -50 and c0 == (1 << 60) + 3 + r and str(d1) == "-0.0" and c1 == -1 - r
        assert g["kl"].dtype == torch.float32 and tuple(g["kl"].shape) == (world, 3, 5, 2)
        for r in range(world):
            assert bool((g["kl"][r, ..., 0] == r + 1).all()) and bool(torch.isinf(g["kl"][r, ..., 1]).all())


def test_all_gather_records_is_the_identity_without_a_group():
    assert not parallel.collectives_active()
    t = record(0)
    out = parallel.all_gather_records(t)
    assert tuple(out.shape) == (1, 4) and torch.equal(out[0], t) and out.data_ptr() == t.data_ptr()
    assert T.all_gather_records is parallel.all_gather_records


def test_batch_scope_values_and_the_tie_count_bound():
    assert ops.phased_scope("global", "t") is False and ops.phased_scope("shard", "t") is False        # no process group here: the unsplit path
    for bad in ("rank", "", None, "Global", 1):
        with pytest.raises(T.TfcError, match="batch_scope"):
            ops.phased_scope(bad, "t")
    ops.check_mask_tie_range(8, 32, 256, 256)                       # exactly 2^24: the largest batch whose counts stay exact
    ops.check_mask_tie_range(1, 1, 8, 8)
    for world, N, H, W in ((8, 33, 256, 256), (64, 5, 256, 256), (2, 1, 4096, 4096 // 2 + 1)):
        assert world * N * H * W > 1 << 24
        with pytest.raises(T.TfcError, match="2\\^24"):
            ops.check_mask_tie_range(world, N, H, W)
    x = torch.zeros(2, 3, 8, 8)
    for call in (lambda: ops.mask_fwd(x, batch_scope="all"), lambda: T.mask_maker(x, batch_scope="all"), lambda: T.mask_l1_loss(x, x, batch_scope="all"),
                 lambda: T.regional_fft_loss(x, x, "kl", batch_scope="all"),
                 lambda: ops.batch_kl_sum(x, x, x, 1.0, x, batch_scope="all")):
        with pytest.raises(T.TfcError, match="batch_scope"):     # refused before anything else is looked at
            call()
    G, D = T.GeneratorUNet((3, 256, 256)), T.Discriminator1((3, 256, 256))
    with pytest.raises(T.TfcError, match="batch_scope"):
        T.TrainStep(G, D, patches=4, batch_scope="all")
