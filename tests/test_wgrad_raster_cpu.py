"""The wgrad grid: plan and block decode, as the launcher and the kernel run
them (conv_igemm_wgrad_config, conv_wgrad_block_coords).

The kernel launches a 1-D grid and decodes a block id into (ktile, ctile,
rs, chunk) through an XCD-contiguous logical id with the chunk slowest. For
every body conv of ResNet-18/34/50 at 224x224, batch 1 and batch 96, and for
hand-picked grids whose size is 0, 1 and 7 modulo the 8 XCDs, the decode must
hit every block exactly once and hand each `bid % 8` class one contiguous
logical range. The (FT, mch, nch) plan of the ten ResNet-34 batch-96 shapes
is pinned: each was measured (profiles/wgrad_raster.md), and a change to the
chunk rule must show up here. CPU-only arithmetic.
"""

import pytest

from fluxdistributed_amd.ops.native import load_native

C_ = load_native()
if C_ is None:  # pragma: no cover
    pytest.skip("native extension not built", allow_module_level=True)

# (M, C, K, R, S), M = batch * P * Q of the conv's output
_STAGES = [
    # (P*Q, [(C, K, R), ...]) for ResNet-18/34 and ResNet-50 body convs
    (3136, [(64, 64, 1), (64, 64, 3), (64, 256, 1), (256, 64, 1),
            (256, 128, 1)]),
    (784, [(64, 128, 1), (64, 128, 3), (128, 128, 3), (128, 512, 1),
           (256, 512, 1), (512, 128, 1), (512, 256, 1)]),
    (196, [(128, 256, 1), (128, 256, 3), (256, 256, 3), (256, 1024, 1),
           (512, 1024, 1), (1024, 256, 1), (1024, 512, 1)]),
    (49, [(256, 512, 1), (256, 512, 3), (512, 512, 3), (512, 2048, 1),
          (1024, 2048, 1), (2048, 512, 1)]),
]
BODY = sorted((b * pq, c, k, r, r) for b in (1, 96) for pq, convs in _STAGES
              for (c, k, r) in convs)

# (ktiles, ctiles, RS, nch): nwg % 8 == 0, 1, 7; stem-like (ctiles 1, RS 7);
# a grid smaller than the XCD count; a single block
HAND_GRIDS = [
    (2, 2, 9, 4),     # 144, % 8 == 0
    (1, 1, 9, 1),     # 9,   % 8 == 1
    (3, 1, 9, 3),     # 81,  % 8 == 1
    (1, 1, 1, 7),     # 7,   % 8 == 7
    (5, 3, 1, 1),     # 15,  % 8 == 7
    (1, 1, 7, 9),     # 63,  % 8 == 7
    (4, 2, 9, 11),    # 792, % 8 == 0
    (1, 1, 7, 25),    # the stem at batch 8: 175, % 8 == 7
    (1, 1, 1, 1),
    (1, 1, 3, 1),
]

# the shipped plan of the ten ResNet-34 batch-96 body shapes: (FT, mch, nch)
PINNED = {
    (301056, 64, 64, 3, 3): (2, 3584, 84),
    (75264, 64, 128, 3, 3): (2, 1792, 42),
    (75264, 64, 128, 1, 1): (2, 448, 168),
    (75264, 128, 128, 3, 3): (4, 1344, 56),
    (18816, 128, 256, 3, 3): (2, 1920, 10),
    (18816, 128, 256, 1, 1): (2, 448, 42),
    (18816, 256, 256, 3, 3): (4, 1344, 14),
    (4704, 256, 512, 3, 3): (4, 704, 7),
    (4704, 256, 512, 1, 1): (2, 448, 11),
    (4704, 512, 512, 3, 3): (4, 1600, 3),
}


def _check_grid(ktiles, ctiles, RS, nch):
    nwg = ktiles * ctiles * RS * nch
    seen = set()
    logical = [[] for _ in range(8)]
    for bid in range(nwg):
        kt, ct, rs, ch = C_.conv_wgrad_block_coords(bid, ktiles, ctiles, RS,
                                                    nch)
        assert 0 <= kt < ktiles and 0 <= ct < ctiles
        assert 0 <= rs < RS and 0 <= ch < nch
        seen.add((kt, ct, rs, ch))
        logical[bid % 8].append(((ch * RS + rs) * ctiles + ct) * ktiles + kt)
    # a bijection: nwg decodes, nwg distinct blocks
    assert len(seen) == nwg
    # blocks that share bid % 8 (an XCD) own one contiguous logical range,
    # in dispatch order, and the eight ranges tile [0, nwg)
    start = 0
    for ids in logical:
        assert ids == list(range(start, start + len(ids)))
        start += len(ids)
    assert start == nwg


def test_body_list_covers_the_models():
    assert len(BODY) == 50
    assert set(PINNED) <= set(BODY)


@pytest.mark.parametrize("shape", BODY)
def test_plan_and_decode_cover_the_grid(shape):
    M, C, K, R, S = shape
    ft, mch, nch, nwg = C_.conv_igemm_wgrad_config(*shape)
    assert ft in (2, 4)
    tile = 32 * ft
    assert K % tile == 0 and C % tile == 0
    # whole 64-pixel K-steps, and chunks that cover M with none empty
    assert mch % 64 == 0
    assert nch * mch >= M > (nch - 1) * mch
    assert nwg == (K // tile) * (C // tile) * R * S * nch
    # up to 4096 pixels: one or two chunks, an order-independent fp32 sum
    if M <= 4096:
        assert (mch, nch) == (2048, (M + 2047) // 2048)
    # beyond: one resident wave at the most, unless at the 448-pixel floor
    elif mch > 448:
        assert nwg <= 256 * (2 if ft == 4 else 3)
    _check_grid(K // tile, C // tile, R * S, nch)


@pytest.mark.parametrize("grid", HAND_GRIDS)
def test_decode_hand_picked_grids(grid):
    _check_grid(*grid)


def test_hand_picked_grids_cover_the_remainders():
    rem = {(kt * ct * rs * nch) % 8 for kt, ct, rs, nch in HAND_GRIDS}
    assert {0, 1, 7} <= rem


def test_block_outside_the_grid_is_refused():
    with pytest.raises(RuntimeError, match="outside the grid"):
        C_.conv_wgrad_block_coords(9, 1, 1, 9, 1)
    with pytest.raises(RuntimeError, match="bad grid"):
        C_.conv_wgrad_block_coords(0, 0, 1, 9, 1)


@pytest.mark.parametrize("shape", sorted(PINNED))
def test_wgrad_plan_is_pinned(shape):
    assert tuple(C_.conv_igemm_wgrad_config(*shape))[:3] == PINNED[shape]
