"""CPU: the host-side tables and checks of ``mrisr.fit`` - learning-rate and EMA-decay tables, the epoch permutation with its
per-rank shards, and the configuration values ``fit`` refuses before any GPU work."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mri-diffusion-superresolution_amd"))
sys.path.insert(0, ROOT)


def test_lr_and_ema_tables_equal_the_eager_schedules():
    import mrisr
    from mrisr.fit import ema_decay_table, lr_table
    from mrisr.train import _FlatAdamW
    cfg = mrisr.TrainConfig(max_train_steps=40, lr_warmup_steps=7, learning_rate=3e-4)
    tab = lr_table(cfg)
    assert len(tab) == 40
    assert tab == [mrisr.cosine_lr(s, 3e-4, 7, 40) for s in range(40)]
    assert tab[0] == 0.0 and max(tab) == pytest.approx(3e-4)
    # as float32 (what the device table holds) each entry is the value the eager path hands to C as c_float
    assert np.array_equal(np.asarray(tab, np.float32), np.asarray([np.float32(x) for x in tab]))
    cfg.lr_scheduler_name = "constant"
    assert lr_table(cfg) == [3e-4] * 40
    cfg.scale_lr, cfg.train_batch_size, cfg.gradient_accumulation_steps = True, 2, 3
    assert lr_table(cfg, world=2)[5] == pytest.approx(3e-4 * 12)
    dec = ema_decay_table(40)
    assert dec == [_FlatAdamW.ema_decay_at(s + 1) for s in range(40)]
    assert dec[0] == 0.0 and dec[1] == pytest.approx(2 / 11)


def test_epoch_permutation_sharding_and_drop_last():
    from mrisr.dist import shard_range
    from mrisr.fit import epoch_index_table
    N, B, world, seed = 23, 3, 2, 5
    per_rank = (N // world) // B  # 3 micro-batches per rank per epoch: 2 of each rank's 11 / 12 items are dropped
    n_micro = 4 * per_rank
    tabs = [epoch_index_table(N, B, world, r, seed, n_micro) for r in range(world)]
    for r, (idx, ep) in enumerate(tabs):
        assert idx.shape == (n_micro, B) and idx.dtype == np.int32
        assert list(ep) == [e for e in range(4) for _ in range(per_rank)]
    for e in range(4):
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed + e)).numpy()
        seen = []
        for r, (idx, ep) in enumerate(tabs):
            got = idx[ep == e].reshape(-1)
            lo, hi = shard_range(N, world, r)
            assert list(got) == list(perm[lo:hi][:per_rank * B])  # the rank's shard, in permutation order, drop-last
            assert len(set(got)) == len(got)
            seen.append(set(got))
        assert not (seen[0] & seen[1])  # shards of one epoch are disjoint
    # consecutive epochs are different shuffles; the table is a pure function of its arguments
    assert not np.array_equal(tabs[0][0][:per_rank], tabs[0][0][per_rank:2 * per_rank])
    assert np.array_equal(epoch_index_table(N, B, world, 0, seed, n_micro)[0], tabs[0][0])
    with pytest.raises(ValueError):
        epoch_index_table(5, 3, 2, 0, 0, 1)  # not one whole micro-batch per rank


@pytest.mark.parametrize("change,match", [
    ({"ddpm_scheduler_prediction_type": "v_prediction"}, "epsilon"),
    ({"lr_scheduler_name": "polynomial"}, "lr_scheduler_name"),
    ({"proportion_empty_prompts": 0.1}, "empty prompt"),
    ({"gradient_accumulation_steps": 0}, "gradient_accumulation_steps"),
])
def test_bad_config_is_refused_before_gpu_work(change, match):
    import mrisr
    cfg = mrisr.TrainConfig(**change)
    embeds = {"a T2 slice": torch.zeros(4, 8)}
    if match != "empty prompt":
        embeds[""] = torch.zeros(4, 8)
    # unet / vae / dataset are never touched: the check runs first (no GPU on this machine)
    with pytest.raises(ValueError, match=match):
        mrisr.fit(cfg, None, None, [], embeds)


def test_check_config_accepts_the_notebook_defaults():
    import mrisr
    from mrisr.fit import check_config
    check_config(mrisr.TrainConfig(), {"": torch.zeros(4, 8), "x": torch.zeros(4, 8)})
