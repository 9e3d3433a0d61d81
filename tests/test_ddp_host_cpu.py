"""CPU: the host side of distributed training (xmh/ddp.py, the runners): the bucket's layout, table and chunk map, the train
loader's sampler, and the refusals that stay."""
import types

import numpy as np
import pytest
import torch


def test_bucket_offsets_flag_tail_and_chunk_map_with_a_missing_gradient():
    from xmh import _lib, ddp
    from xmh.optim import BertAdam
    chunk = int(_lib.lib.xmh_bertadam_chunk())
    numels = [1, 64, 65, chunk, 2 * chunk + 1, 7]
    offsets, tail, total = ddp.bucket_layout(numels)
    assert offsets == [0, 64, 128, 256, 256 + chunk, 256 + chunk + 2 * chunk + 64]
    assert tail == offsets[-1] + 64 and total == tail + 64                               # six flags, rounded up to 64 floats
    assert all(o % 64 == 0 for o in offsets + [tail, total])
    for o, n, nxt in zip(offsets, numels, offsets[1:] + [tail]):
        assert o + n <= nxt < o + n + 64                                                 # no overlap, under 64 floats of padding
    pointers = [4096, 8192, None, 12288, 16384, 20480]                                   # parameter 2 has no gradient on this rank
    table = ddp.bucket_table(pointers, numels)
    assert table.dtype.itemsize == 40 and table["t"].tolist() == [4096, 8192, 0, 12288, 16384, 20480]
    assert table["offset"].tolist() == offsets and table["numel"].tolist() == numels
    assert table["flag"].tolist() == [1.0, 1.0, 0.0, 1.0, 1.0, 1.0]
    assert table["flag_at"].tolist() == [tail + i for i in range(6)] and not table["reserved"].any()
    plain = ddp.bucket_table(pointers, numels, flags=False)                              # the parameter broadcast carries no tail
    assert plain["flag_at"].tolist() == [-1] * 6 and not plain["flag"].any()
    cmap = ddp.chunk_map(numels, chunk)
    assert cmap["tensor"].tolist() == [0, 1, 2, 3, 4, 4, 4, 5]
    assert cmap["start"].tolist() == [0, 0, 0, 0, 0, chunk, 2 * chunk, 0]
    assert cmap["first_chunk"].tolist() == [0, 1, 2, 3, 4, 4, 4, 7]
    opt = BertAdam([torch.nn.Parameter(torch.zeros(1))], lr=0.1)                          # the optimiser's map: one layout for both
    opt._mirrors()
    assert np.array_equal(opt._chunk_map(numels, chunk), cmap)
    assert len(ddp.chunk_map([], chunk)) == 0 and ddp.bucket_layout([]) == ([], 0, 0)
    with pytest.raises(ValueError, match="empty"):
        ddp.bucket_layout([3, 0])


class _Split(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i

    def get_all_label(self):
        return torch.zeros(self.n, 4)


@pytest.mark.parametrize("train_num", [60, 61])
@pytest.mark.parametrize("world", [2, 3])
def test_the_distributed_train_loader_shards_the_training_set(train_num, world):
    """every rank gets ceil(train_num / W) indices (the sampler pads: the same number of steps everywhere), the union is the set, and
    the batch size is batch_size // W"""
    from xmh.runners.base import BaseTrainer
    per_rank = -(-train_num // world)
    seen = []
    for rank in range(world):
        t = types.SimpleNamespace(distributed=True, rank=rank, world_size=world, logger=types.SimpleNamespace(info=lambda *a: None))
        BaseTrainer.build_loader(t, _Split(train_num), _Split(10), _Split(20), 8, 0, False, True)
        idx = [int(i) for batch in t.train_loader for i in batch]
        assert len(idx) == per_rank and t.train_loader.batch_size == 8 // world
        assert len(t.train_loader) == -(-per_rank // (8 // world))
        again = [int(i) for batch in t.train_loader for i in batch]
        assert again == idx                                                              # no set_epoch: every epoch draws the same order
        seen.append(idx)
    assert set(i for idx in seen for i in idx) == set(range(train_num))
    assert sum(len(idx) for idx in seen) == per_rank * world
    single = types.SimpleNamespace(distributed=False, rank=0, world_size=1, logger=types.SimpleNamespace(info=lambda *a: None))
    BaseTrainer.build_loader(single, _Split(train_num), _Split(10), _Split(20), 8, 0, False, False)
    assert [int(i) for b in single.train_loader for i in b] == list(range(train_num))    # one process: as before


def test_methods_with_per_rank_state_still_refuse_a_distributed_epoch():
    from xmh.runners.methods import DCMHTTrainer, DIMCHTrainer, DNPHTrainer, MITHTrainer, TwDHTrainer, UMoEDTrainer
    ns = types.SimpleNamespace(distributed=True)
    for call, words in ((MITHTrainer.train_epoch_towers, ("feature bank", "buffer broadcast")),
                        (DNPHTrainer.train_epoch, ("noise assignment", "buffer broadcast")),
                        (DCMHTTrainer.train_epoch, ("BatchNorm", "no process group")),     # a model that build_model did not prepare
                        (TwDHTrainer.train_epoch_codes, ("float64",)),
                        (DIMCHTrainer.train_epoch, ("float64",)),
                        (UMoEDTrainer.train_epoch_decoder, ("float64",))):
        with pytest.raises(NotImplementedError) as err:
            call(ns, 0)
        assert all(w in str(err.value) for w in words) and "distributed=True" in str(err.value), str(err.value)
