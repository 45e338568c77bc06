"""The unstaged ("direct") branch of the row binning's emission tail (rb_emit_chunk, ggd_rowbin.hip): a chunk whose output does
not fit the LDS staging buffer (RB_STAGE1 = 4096 row entries at level 1, RB_STAGE = 4096 instances at level 2) is written straight
to memory behind the bound check instead of being staged and copied out as runs.  The ordinary test scenes have small splats and
never get there; these two have large ones on a 16 x 16-tile grid:
  lsm = -4.0   level-1 chunks 0 and 1 (1024 Gaussians, about 5 600 row entries each) are direct, the ragged chunk 2 (552 Gaussians,
               about 3 000) is staged -- both branches in one frame; every tile row's level-2 block is direct
  lsm = -3.5   every chunk of either level is direct
Every case asserts that premise on the CPU first, from the oracle's rects in depth order (the chunks are 1024 consecutive depth
ranks at level 1, 1024 consecutive entries of a tile row at level 2), then renders on one of the three paths that own an emission
site and compares every frame's num_rendered, sorted list and ranges with the oracle's bit for bit:
  counted     folded front end behind the two-launch sort: rb_level1_counted_kernel (GGD_STAT_L1_COUNTED_FRAMES advances)
  look-back   the same with GGD_OPT_L1_COUNTED = 0: rb_level1_kernel and rb_scatter2_kernel<true>
              (GGD_STAT_SCAN_IN_SCATTER_FRAMES advances)
  plain       GGD_OPT_FOLD = 0: rb_count1 / rb_scan1 / rb_scatter1, rb_scan2 and rb_scatter2_kernel<false>"""
import functools

import numpy as np
import pytest

from _util import run_oracle, depth_keys
from test_level1_counted_gpu import CHUNK, on_screen_scene, _ctx, _frame, _until_two_launches

pytestmark = pytest.mark.gpu

STAGE1 = STAGE2 = 4096          # RB_STAGE1, RB_STAGE
SIZE = 256                      # 16 x 16 tiles


def _chunk_sums(v):
    return np.add.reduceat(v, np.arange(0, len(v), CHUNK)) if len(v) else np.zeros(0, np.int64)


def emission_counts(o, size=SIZE):
    """(row entries of every level-1 chunk, instances of every level-2 block) of the oracle frame `o`"""
    vis = np.nonzero(o["radii"] > 0)[0]
    order = vis[np.argsort(depth_keys(o), kind="stable")]          # (depth bits, index)
    r = o["rect"][order].astype(np.int64)                           # x0, y0, x1, y1
    w, h = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    live = (w > 0) & (h > 0)
    l1 = _chunk_sums(np.where(live, h, 0))
    l2 = np.concatenate([_chunk_sums(w[live & (r[:, 1] <= y) & (y < r[:, 3])]) for y in range((size + 15) // 16)])
    assert l1.sum() == h[live].sum() and l2.sum() == o["num_rendered"]
    return l1, l2


@functools.lru_cache(maxsize=None)
def scene(lsm):
    d = on_screen_scene(2600, SIZE, seed=21, lsm=lsm)
    o = run_oracle(d)
    return d, o, emission_counts(o)


def assert_premise(lsm):
    d, o, (l1, l2) = scene(lsm)
    assert len(l1) == 3, "three level-1 chunks, the last one ragged"
    if lsm == -4.0:     # both branches of level 1 in one frame
        assert (l1 > STAGE1).any() and ((l1 > 0) & (l1 <= STAGE1)).any(), l1
    else:               # every chunk of level 1 is direct
        assert (l1 > STAGE1).all(), l1
    assert (l2 > STAGE2).any(), l2
    return d, o


def _scan_in_scatter_frames():
    _capi, ctx = _ctx()
    return ctx.get_option(_capi.STAT_SCAN_IN_SCATTER_FRAMES)


def _counted(d, o):
    _capi, ctx = _ctx()
    assert ctx.get_option(_capi.OPT_L1_COUNTED) == 1, "the counted level 1 is the default"
    _until_two_launches(d, o, 1)              # asserts that GGD_STAT_L1_COUNTED_FRAMES advanced by the three frames


def _look_back(d, o):
    _capi, ctx = _ctx()
    s0 = _scan_in_scatter_frames()
    try:
        _until_two_launches(d, o, 0)          # asserts that GGD_STAT_L1_COUNTED_FRAMES stood still
    finally:
        ctx.set_option(_capi.OPT_L1_COUNTED, 1)
    assert _scan_in_scatter_frames() >= s0 + 3, "rb_scatter2_kernel<true> did not run"


def _plain(d, o):
    _capi, ctx = _ctx()
    saved = ctx.get_option(_capi.OPT_FOLD)
    s0 = _scan_in_scatter_frames()
    try:
        ctx.set_option(_capi.OPT_FOLD, 0)
        for i in range(2):
            _frame(d, o, ("plain", i))
    finally:
        ctx.set_option(_capi.OPT_FOLD, saved)
    assert _scan_in_scatter_frames() == s0, "the plain path runs rb_scan2_kernel"


@pytest.mark.parametrize("path", [_counted, _look_back, _plain], ids=["counted", "look-back", "plain"])
@pytest.mark.parametrize("lsm", [-4.0, -3.5], ids=["staged-and-direct", "all-direct"])
def test_chunks_beyond_the_staging_buffer(native_lib, lsm, path):
    d, o = assert_premise(lsm)                # on the CPU, before anything runs on the GPU
    path(d, o)
