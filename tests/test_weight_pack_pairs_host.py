"""mi355_weight_pack_multi_pairs (host only, no GPU): which descriptors of a re-pack list mi355_weight_pack_multi takes as a
forward / data-gradient pair of one tensor and writes from one read of it.  Pointers are dummies: nothing is launched."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wpack_descs as W  # noqa: E402
from unet_bssfp_amd import _lib  # noqa: E402

BF16, F32 = _lib.DT_BF16, _lib.DT_F32
SRC, DST = 0x10000, 0x900000          # distinct tensors / buffers: SRC + k * 0x10000, DST + k * 0x10000


def _unrelated(k):
    """a 1x1x1 packing and packings of other tensors: partners of nothing that the tests pair"""
    src, dst = SRC + (100 + k) * 0x10000, DST + (100 + k) * 0x10000
    return [W.pointwise(src, dst, 24, 24, BF16), W.dense_fwd(src, dst, 32, 64, BF16), W.s2d_dgrad(src, dst, 64, 30, 32, BF16)][k % 3]


def test_one_forward_and_data_gradient_pair():
    assert W.pair_count([W.dense_fwd(SRC, DST, 48, 24, BF16, cinp=32), W.dense_dgrad(SRC, DST + 0x10000, 48, 24, BF16)]) == 1
    assert W.pair_count([W.dense_dgrad(SRC, DST + 0x10000, 48, 24, BF16), W.dense_fwd(SRC, DST, 48, 24, BF16, cinp=32)]) == 1
    assert W.pair_count([W.s2d_dgrad(SRC, DST + 0x10000, 64, 30, 32, F32), W.s2d_fwd(SRC, DST, 64, 30, 32, F32)]) == 1


def test_pair_survives_twenty_descriptors_between_its_members():
    """the members fall into different 16-descriptor launch groups of the list"""
    between = [_unrelated(k) for k in range(20)]
    assert W.pair_count(between) == 0
    descs = [W.dense_fwd(SRC, DST, 32, 32, BF16)] + between + [W.dense_dgrad(SRC, DST + 0x10000, 32, 32, BF16)]
    assert W.pair_count(descs) == 1
    assert W.pair_count(descs[::-1]) == 1


def test_forward_alone_has_no_partner():
    assert W.pair_count([W.dense_fwd(SRC, DST, 32, 32, BF16)]) == 0
    assert W.pair_count([W.s2d_fwd(SRC, DST, 24, 16, 16, BF16)]) == 0
    # two forward packings of one tensor (different cinp) are no pair, and neither are packings of two tensors
    assert W.pair_count([W.dense_fwd(SRC, DST, 32, 32, BF16), W.dense_fwd(SRC, DST + 0x10000, 32, 32, BF16, cinp=64)]) == 0
    assert W.pair_count([W.dense_fwd(SRC, DST, 32, 32, BF16), W.dense_dgrad(SRC + 0x10000, DST + 0x10000, 32, 32, BF16)]) == 0
    # space-to-depth partners must share s2d_cp
    assert W.pair_count([W.s2d_fwd(SRC, DST, 24, 16, 16, BF16), W.s2d_dgrad(SRC, DST + 0x10000, 24, 16, 32, BF16)]) == 0


def test_partners_of_different_dtype_are_not_paired():
    assert W.pair_count([W.dense_fwd(SRC, DST, 32, 32, BF16), W.dense_dgrad(SRC, DST + 0x10000, 32, 32, F32)]) == 0
    assert W.pair_count([W.s2d_fwd(SRC, DST, 24, 16, 16, F32), W.s2d_dgrad(SRC, DST + 0x10000, 24, 16, 16, BF16)]) == 0


def test_channel_slice_next_to_its_full_tensor_partner_is_not_paired():
    full_fwd, full_dgrad = W.dense_fwd(SRC, DST, 32, 96, BF16), W.dense_dgrad(SRC, DST + 0x10000, 32, 96, BF16)
    for c_off, c_n in ((0, 32), (32, 64)):
        assert W.pair_count([W.dense_fwd(SRC, DST + 0x20000, 32, 96, BF16, c_off=c_off, c_n=c_n), full_dgrad]) == 0
        assert W.pair_count([full_fwd, W.dense_dgrad(SRC, DST + 0x20000, 32, 96, BF16, c_off=c_off, c_n=c_n)]) == 0
        # nor are the two slice packings of one slice: their strides are not those of a dense tensor
        assert W.pair_count([W.dense_fwd(SRC, DST + 0x20000, 32, 96, BF16, c_off=c_off, c_n=c_n),
                             W.dense_dgrad(SRC, DST + 0x30000, 32, 96, BF16, c_off=c_off, c_n=c_n)]) == 0


def test_one_dense_pair_and_one_space_to_depth_pair():
    descs = [W.dense_fwd(SRC, DST, 32, 18, BF16), W.s2d_dgrad(SRC + 0x10000, DST + 0x10000, 64, 30, 32, BF16),
             W.pointwise(SRC + 0x20000, DST + 0x20000, 24, 24, BF16),
             W.dense_dgrad(SRC, DST + 0x30000, 32, 18, BF16), W.s2d_fwd(SRC + 0x10000, DST + 0x40000, 64, 30, 32, BF16)]
    assert W.pair_count(descs) == 2


def test_query_validates_like_the_launcher():
    lib = _lib.load()
    assert lib.mi355_weight_pack_multi_pairs(None, 1) < 0
    assert b"weight_pack_multi_pairs: bad argument" in lib.mi355_last_error()
    assert W.pair_count([W.dense_fwd(0, DST, 32, 32, BF16)]) < 0
    assert b"weight_pack: null pointer" in lib.mi355_last_error()
