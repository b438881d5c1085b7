"""The conv plan is pinned: (BM, BN, SK, ring) of every body conv of
ResNet-18/34/50 at 224x224, batch 1 and batch 96, as
conv_igemm_fwd_config(M, C, K, R, S) reports it (M = batch * P * Q).

The kernels behind each entry are chosen and measured; a change to the plan
(tile rule, split-K thresholds 48/192/384, ring thresholds 576/512) must show
up here. CPU-only arithmetic; FLUXDIST_CONV_BK32 must be unset (the default,
rings on), since the extension reads it once per process.
"""

import os

import pytest

from fluxdistributed_amd.ops.native import load_native

C_ = load_native()
if C_ is None:  # pragma: no cover
    pytest.skip("native extension not built", allow_module_level=True)
if "FLUXDIST_CONV_BK32" in os.environ:  # pragma: no cover
    pytest.skip("pinned with FLUXDIST_CONV_BK32 unset", allow_module_level=True)

# (M, C, K, R, S): (BM, BN, SK, ring)
PLAN = {
    (49, 256, 512, 1, 1): (128, 128, 1, False),
    (49, 256, 512, 3, 3): (128, 128, 1, False),
    (49, 512, 512, 3, 3): (128, 128, 4, False),
    (49, 512, 2048, 1, 1): (128, 128, 1, False),
    (49, 1024, 2048, 1, 1): (128, 128, 1, False),
    (49, 2048, 512, 1, 1): (128, 128, 1, False),
    (196, 128, 256, 1, 1): (128, 128, 1, False),
    (196, 128, 256, 3, 3): (128, 128, 1, False),
    (196, 256, 256, 3, 3): (128, 128, 1, False),
    (196, 256, 1024, 1, 1): (128, 128, 1, False),
    (196, 512, 1024, 1, 1): (128, 128, 1, False),
    (196, 1024, 256, 1, 1): (128, 128, 1, False),
    (196, 1024, 512, 1, 1): (128, 128, 1, False),
    (784, 64, 128, 1, 1): (128, 128, 1, False),
    (784, 64, 128, 3, 3): (128, 128, 1, False),
    (784, 128, 128, 3, 3): (128, 128, 1, False),
    (784, 128, 512, 1, 1): (128, 128, 1, False),
    (784, 256, 512, 1, 1): (128, 128, 1, False),
    (784, 512, 128, 1, 1): (128, 128, 1, False),
    (784, 512, 256, 1, 1): (128, 128, 1, False),
    (3136, 64, 64, 1, 1): (256, 64, 1, False),
    (3136, 64, 64, 3, 3): (256, 64, 1, False),
    (3136, 64, 256, 1, 1): (128, 128, 1, False),
    (3136, 256, 64, 1, 1): (256, 64, 1, False),
    (3136, 256, 128, 1, 1): (128, 128, 1, False),
    (4704, 256, 512, 1, 1): (128, 128, 1, False),
    (4704, 256, 512, 3, 3): (128, 128, 1, False),
    (4704, 512, 512, 3, 3): (128, 128, 4, True),
    (4704, 512, 2048, 1, 1): (128, 128, 1, True),
    (4704, 1024, 2048, 1, 1): (128, 128, 1, True),
    (4704, 2048, 512, 1, 1): (128, 128, 1, False),
    (18816, 128, 256, 1, 1): (128, 128, 1, False),
    (18816, 128, 256, 3, 3): (128, 128, 1, False),
    (18816, 256, 256, 3, 3): (128, 128, 1, False),
    (18816, 256, 1024, 1, 1): (128, 128, 1, True),
    (18816, 512, 1024, 1, 1): (128, 128, 1, True),
    (18816, 1024, 256, 1, 1): (128, 128, 1, False),
    (18816, 1024, 512, 1, 1): (128, 128, 1, True),
    (75264, 64, 128, 1, 1): (128, 128, 1, True),
    (75264, 64, 128, 3, 3): (128, 128, 1, True),
    (75264, 128, 128, 3, 3): (128, 128, 1, True),
    (75264, 128, 512, 1, 1): (128, 128, 1, True),
    (75264, 256, 512, 1, 1): (128, 128, 1, True),
    (75264, 512, 128, 1, 1): (128, 128, 1, True),
    (75264, 512, 256, 1, 1): (128, 128, 1, True),
    (301056, 64, 64, 1, 1): (256, 64, 1, True),
    (301056, 64, 64, 3, 3): (256, 64, 1, True),
    (301056, 64, 256, 1, 1): (128, 128, 1, True),
    (301056, 256, 64, 1, 1): (256, 64, 1, True),
    (301056, 256, 128, 1, 1): (128, 128, 1, True),
}


def test_plan_covers_the_models():
    assert len(PLAN) == 50
    # both tiles, split and unsplit K, and both ring states occur
    assert {v[:2] for v in PLAN.values()} == {(128, 128), (256, 64)}
    assert {v[2] for v in PLAN.values()} == {1, 4}
    assert {v[3] for v in PLAN.values()} == {False, True}


@pytest.mark.parametrize("shape", sorted(PLAN))
def test_conv_plan_is_pinned(shape):
    assert tuple(C_.conv_igemm_fwd_config(*shape)) == PLAN[shape]
