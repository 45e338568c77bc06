"""The cross-lane primitives of csrc/ggd_lanes.h through ggd_selftest_lanes: the 64-lane inclusive scan on DPP,
the wave sum and maximum, lane_xor<1 .. 32>, lane_pair_sum<16 / 32>, wave_pick on v_readlane and the 64 x 64 bit-matrix transpose on
the lane-block swaps.  Every launch runs 8 waves; the kernel writes each primitive next to the __shfl form it replaced, and both
are compared, exactly, with numpy: cumsum per 64 lanes, sum, max, index arithmetic, the transpose of the bit matrix.
Inputs are the smallest that can break a DPP scan or a swap: all zeros, all ones, 0xFFFFFFFF everywhere (wrap-around), negative
ints, one non-zero lane at each seam of the 16-lane rows and the half-waves (0, 15, 16, 31, 32, 47, 48, 63 -- where the row_bcast
masks and the swaps act), seeded random words; for the transpose the identity, one set bit at every (row, column) of those seams and
a seeded random matrix."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WAVES = 8
SEAMS = (0, 15, 16, 31, 32, 47, 48, 63)


def run_selftest(words):
    """words: uint64 [WAVES, 64] -> uint32 [WAVES, 64, LANES_SELFTEST_WORDS]"""
    from gaussian_gan_decoder_amd import _capi
    assert words.shape == (WAVES, 64) and words.dtype == np.uint64
    dev = torch.device("cuda:0")
    ctx = _capi.context_for(dev)
    d_in = torch.from_numpy(words.view(np.int64).copy()).to(dev)
    d_out = torch.full((WAVES, 64, _capi.LANES_SELFTEST_WORDS), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.ggd_selftest_lanes(ctx.handle, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream),
                                         C.c_void_p(d_in.data_ptr()), C.c_void_p(d_out.data_ptr()), WAVES))
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32)


def transpose_bits(words):
    """rows of a 64 x 64 bit matrix (bit b of word i = M[i][b]) -> its columns (bit i of word b = M[i][b])"""
    m = (words[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)          # m[i][b]
    return (m.T << np.arange(64, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)   # word b: sum over i of m[i][b] << i


def check(words):
    out = run_selftest(words)
    lanes = np.arange(64)
    x = (words & np.uint64(0xFFFFFFFF)).astype(np.uint32)                                   # [WAVES, 64]
    both = lambda k, want, what: [np.testing.assert_array_equal(out[:, :, k + j], want, err_msg=f"{what} ({n})")
                                  for j, n in ((0, "new form"), (1, "__shfl form"))]
    scan = np.cumsum(x.astype(np.uint64), axis=1).astype(np.uint32)                         # (wraps like the kernel's uint32)
    both(0, scan, "inclusive scan, uint32")
    both(2, np.cumsum(x.view(np.int32).astype(np.int64), axis=1).astype(np.int32).view(np.uint32), "inclusive scan, int")
    both(4, np.broadcast_to(scan[:, 63:64], x.shape), "wave sum")
    both(6, np.broadcast_to(x.max(axis=1, keepdims=True), x.shape), "wave max")
    for k, d in enumerate((1, 2, 4, 8, 16, 32)):
        np.testing.assert_array_equal(out[:, :, 8 + k], x[:, lanes ^ d], err_msg=f"lane_xor<{d}>")
        np.testing.assert_array_equal(out[:, :, 14 + k], x[:, lanes ^ d], err_msg=f"__shfl_xor {d}")
    pick = np.broadcast_to(x[:, None, :], (WAVES, 64, 64))                                  # word 20 + c of every lane: x of lane c
    np.testing.assert_array_equal(out[:, :, 20:84], pick, err_msg="wave_pick")
    np.testing.assert_array_equal(out[:, :, 84:148], pick, err_msg="__shfl")
    want_t = np.stack([transpose_bits(words[w]) for w in range(WAVES)])
    for k, n in ((148, "new form"), (150, "__shfl form")):
        got = out[:, :, k].astype(np.uint64) | (out[:, :, k + 1].astype(np.uint64) << np.uint64(32))
        np.testing.assert_array_equal(got, want_t, err_msg=f"transpose ({n})")
    np.testing.assert_array_equal(out[:, :, 152], x + x[:, lanes ^ 16], err_msg="lane_pair_sum<16>")
    np.testing.assert_array_equal(out[:, :, 153], x + x[:, lanes ^ 32], err_msg="lane_pair_sum<32>")
    np.testing.assert_array_equal(out[:, 63, 154], x.max(axis=1), err_msg="wave_max_lane63")
    np.testing.assert_array_equal(out[:, 63, 155], scan[:, 63], err_msg="wave_sum_lane63")


def const_words(lo):
    return np.full((WAVES, 64), lo, dtype=np.uint64)


def test_transpose_reference_is_a_transpose():
    """the numpy reference itself: an involution that moves bit (i, b) to (b, i)"""
    rng = np.random.default_rng(5)
    w = rng.integers(0, 2**64, size=64, dtype=np.uint64)
    t = transpose_bits(w)
    np.testing.assert_array_equal(transpose_bits(t), w)
    assert (int(t[7]) >> 50) & 1 == (int(w[50]) >> 7) & 1
    one = np.zeros(64, dtype=np.uint64); one[3] = np.uint64(1) << np.uint64(60)
    want = np.zeros(64, dtype=np.uint64); want[60] = np.uint64(1) << np.uint64(3)
    np.testing.assert_array_equal(transpose_bits(one), want)


@pytest.mark.parametrize("lo", [0, 1, 0xFFFFFFFF], ids=["zeros", "ones", "all-bits"])
def test_constant_words(native_lib, lo):
    check(const_words(lo | (lo << 32)))


def test_negative_ints(native_lib):
    """as int: -1, -2, ... and INT_MIN next to small positives (the int scan; the unsigned max sees them as large words)"""
    w = np.zeros((WAVES, 64), dtype=np.uint64)
    lanes = np.arange(64, dtype=np.int64)
    w[0] = (-(lanes + 1)).astype(np.int32).view(np.uint32)
    w[1] = np.where(lanes % 2 == 0, -7, 5).astype(np.int32).view(np.uint32)
    w[2] = np.where(lanes == 31, -2**31, lanes).astype(np.int32).view(np.uint32)
    w[3] = np.where(lanes % 16 == 15, -1000, 1).astype(np.int32).view(np.uint32)
    w[4:] = (-(lanes[None, :] * np.array([[3], [17], [255], [65537]]))).astype(np.int32).view(np.uint32)
    check(w | (w << np.uint64(32)))


def test_single_lane_at_every_seam(native_lib):
    """one non-zero lane per wave, at the row and half-wave seams: a scan step that skips or doubles a row shows in every lane above"""
    for value in (1, 0x80000001):
        w = np.zeros((WAVES, 64), dtype=np.uint64)
        for k, lane in enumerate(SEAMS):
            w[k, lane] = value
        check(w)


def test_random_words(native_lib):
    rng = np.random.default_rng(20260113)
    check(rng.integers(0, 2**64, size=(WAVES, 64), dtype=np.uint64))
    check(rng.integers(0, 2**16, size=(WAVES, 64), dtype=np.uint64))    # small counts, as the kernels scan them


def test_transpose_identity_and_single_bits(native_lib):
    """the identity, and one set bit at every (row, column) of the seams: 64 matrices, 8 per launch"""
    ident = np.uint64(1) << np.arange(64, dtype=np.uint64)
    w = np.tile(ident, (WAVES, 1))
    w[1] = ident[::-1]                      # the anti-diagonal
    w[2] = ~ident
    check(w)
    for row in SEAMS:
        w = np.zeros((WAVES, 64), dtype=np.uint64)
        for k, col in enumerate(SEAMS):
            w[k, row] = np.uint64(1) << np.uint64(col)
        check(w)
