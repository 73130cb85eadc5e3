"""CPU: the host side of ``mrisr.fit(adapter=...)`` - what it refuses before any GPU work, which checkpoints resume into which
runs, and the C ABI it adds to include/mrisr.h."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mri-diffusion-superresolution_amd"))
sys.path.insert(0, ROOT)


def test_bad_config_with_adapter_raises_before_gpu_work():
    import mrisr
    embeds = {"": torch.zeros(4, 8)}
    for kw in (dict(ddpm_scheduler_prediction_type="v_prediction"), dict(lr_scheduler_name="polynomial"), dict(max_train_steps=0),
               dict(proportion_empty_prompts=2.0)):
        cfg = mrisr.TrainConfig(**kw)
        with pytest.raises(ValueError):
            mrisr.fit(cfg, None, None, [], embeds, adapter=object())


def test_checkpoint_bucket_compatibility():
    from mrisr.fit import check_resume_buckets, trained_buckets
    assert trained_buckets(True, False) == ["lora"]
    assert trained_buckets(False, True) == ["adapter"]
    assert trained_buckets(True, True) == ["lora", "adapter"]
    old = {"step": 20, "seed": 1}  # written before the field existed: a LoRA-only run
    check_resume_buckets(old, ["lora"])
    for other in (["adapter"], ["lora", "adapter"]):
        with pytest.raises(ValueError, match="trained lora"):
            check_resume_buckets(old, other)
    frozen = {"step": 20, "seed": 1, "buckets": ["adapter"]}
    check_resume_buckets(frozen, ["adapter"])
    with pytest.raises(ValueError):
        check_resume_buckets(frozen, ["lora"])
    with pytest.raises(ValueError):
        check_resume_buckets(frozen, ["lora", "adapter"])
    joint = {"step": 20, "seed": 1, "buckets": ["lora", "adapter"]}
    check_resume_buckets(joint, ["adapter", "lora"])
    with pytest.raises(ValueError):
        check_resume_buckets(joint, ["adapter"])


def test_header_declares_the_adapter_loop_entries():
    hdr = open(os.path.join(ROOT, "include", "mrisr.h")).read()
    assert re.search(r"^int mrisr_fit_create_adapter\(mrisr_model\* unet, const mrisr_fit_config\* cfg,", hdr, flags=re.M)
    assert re.search(r"const mrisr_fit_adapter_args\* adapter, mrisr_fit\*\* out\);", hdr)
    assert re.search(r"^int mrisr_fit_make_condition\(mrisr_fit\* f, int step, int micro, void\* out_dev, int form, void\* stream\);",
                     hdr, flags=re.M)
    assert re.search(r"\} mrisr_fit_adapter_args;", hdr)
    from mrisr import _lib
    assert {"mrisr_fit_create_adapter", "mrisr_fit_make_condition"} <= set(_lib.EXPORTS)
