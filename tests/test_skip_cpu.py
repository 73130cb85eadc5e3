"""CPU: the host rule of ``Sampler.run(skip_neutral=True)`` - ``mrisr.step_variants`` on hand-written tables, the
pattern a guidance interval gives, and the refusals that need no device."""
import numpy as np
import pytest

import mrisr
from mrisr import STEP_NO_CONTROLNET as NC, STEP_NO_FEATURES as NF, STEP_REDUCED as R
from mrisr.pipeline import check_skip

NEUTRAL = (1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0)


def sched(*gsphi):
    rows = np.tile(np.float32(NEUTRAL), (len(gsphi), 1))
    for i, v in enumerate(gsphi):
        rows[i, :len(v)] = v
    return rows


def cond(*ca):
    rows = np.zeros((len(ca), 4), dtype=np.float32)
    rows[:, :2] = ca
    return rows


def test_reduced_needs_g_one_and_s_zero():
    rows = sched((1.0, 0.0), (3.0, 0.0), (1.0, 2.0), (1.0, -0.0), (1.0, 0.0, 0.7), (np.float32(1.0) + np.float32(2.0 ** -23), 0.0))
    # K = 3: g == 1 and s == 0; -0.0 is 0; phi does not matter; the float32 next to 1 is not 1
    assert mrisr.step_variants(rows, None, 3, pag=True) == [R, 0, 0, R, R, 0]
    # K = 2, classifier-free guidance: the same rule
    assert mrisr.step_variants(rows, None, 2) == [R, 0, 0, R, R, 0]
    # K = 2, PAG alone: s == 0 alone decides (g of the row is not read: the step forms 1 + s)
    assert mrisr.step_variants(rows, None, 2, pag=True) == [R, R, 0, R, R, R]
    # a plain run has no rows to leave out
    assert mrisr.step_variants(rows, None, 1) == [0] * 6


def test_no_table_nothing_to_skip():
    assert mrisr.step_variants(None, None, 2, True, 4, n_steps=3) == [0, 0, 0]
    assert mrisr.step_variants(None, cond((0.0, 0.0)), 3, True, 2, pag=True) == [NC | NF]  # no schedule table: never reduced
    assert mrisr.step_variants(sched((1.0, 0.0)), None, 2, True, 2) == [R]                  # no conditioning table: both networks run
    with pytest.raises(ValueError, match="n_steps"):
        mrisr.step_variants(None, None, 2)


def test_conditioning_columns_need_their_network():
    rows = cond((0.0, 1.0), (0.5, 0.0), (-0.0, -0.0), (1.0, 1.0))
    assert mrisr.step_variants(None, rows, 1, True, 4) == [NC, NF, NC | NF, 0]
    assert mrisr.step_variants(None, rows, 1, False, 4) == [0, NF, NF, 0]  # c == 0 without a ControlNet: nothing to skip
    assert mrisr.step_variants(None, rows, 1, True, 0) == [NC, 0, NC, 0]   # a == 0 without features
    assert mrisr.step_variants(None, rows, 1) == [0, 0, 0, 0]


def test_both_tables_combine_per_step():
    s = sched((3.0, 0.0), (1.0, 0.0), (1.0, 0.0))
    c = cond((1.0, 1.0), (0.0, 1.0), (0.0, 0.0))
    assert mrisr.step_variants(s, c, 2, True, 1) == [0, R | NC, R | NC | NF]
    with pytest.raises(ValueError, match="agree"):
        mrisr.step_variants(s, c[:2], 2, True, 1)
    for bad in (0, 4, True, 2.0):
        with pytest.raises(ValueError, match="K must be"):
            mrisr.step_variants(s, None, bad)
    with pytest.raises(ValueError, match="pag=True"):
        mrisr.step_variants(s, None, 1, pag=True)
    with pytest.raises(ValueError, match=r"\[n, 8\]"):
        mrisr.step_variants(c, None, 2)
    with pytest.raises(ValueError, match=r"\[n, 4\]"):
        mrisr.step_variants(None, s, 2)


def test_guidance_interval_at_five_steps():
    """guidance_interval=(0.4, 0.8) at n = 5: guided steps {2, 3}, reduced steps {0, 1, 4}."""
    ts = np.array([801, 601, 401, 201, 1])
    rows = mrisr.step_schedule(ts, guidance_scale=3.0, guidance_rescale=0.7, guidance_interval=(0.4, 0.8))
    v = mrisr.step_variants(rows, None, 2)
    assert [i for i, x in enumerate(v) if x == 0] == [2, 3] and [i for i, x in enumerate(v) if x == R] == [0, 1, 4]
    # control_guidance_end = 0.6 and adapter_conditioning_factor = 0.4: 3 ControlNet steps, 2 feature steps
    c = mrisr.conditioning_schedule(5, control_guidance_end=0.6, adapter_conditioning_factor=0.4)
    v = mrisr.step_variants(None, c, 1, True, 4)
    assert v == [0, 0, NF, NC | NF, NC | NF]


def test_refusals():
    assert check_skip(False) is False and check_skip(True) is True and check_skip(np.bool_(True)) is True
    assert check_skip(False, cache_interval=3) is False  # the default with a cache: nothing to refuse
    with pytest.raises(ValueError, match="feature cache"):
        check_skip(True, cache_interval=2)
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="must be a bool"):
            check_skip(bad)
