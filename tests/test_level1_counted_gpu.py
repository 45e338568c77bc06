"""Level 1 of the row binning without its look-back (rb_level1_counted_kernel, GGD_OPT_L1_COUNTED): on frames
of the two-launch depth sort the finish launch counts every bucket's row entries -- per bucket, and in front of every 1024-rank
chunk boundary inside a bucket -- and level 1 sums those finished rows.  Every case
  * asserts its premise on the CPU, from the oracle's depth keys laid over the window the host will fit (_util.msd_window):
    which bucket holds which depth rank, where the chunk boundaries fall;
  * arms the two-launch sort (setting GGD_OPT_MSD_SORT restarts the speculation: 8 frames form the window) and renders until
    three frames have run in two launches: every frame's num_rendered, sorted list and ranges equal the oracle's, the image
    matches it, GGD_STAT_L1_COUNTED_FRAMES advanced with GGD_STAT_MSD_FRAMES and nothing was rendered again;
  * renders the same frames with GGD_OPT_L1_COUNTED = 0 (the look-back kernel; the counter stands still) on the same context
    and compares the binning buffer and the ranges bit for bit.
Shapes are the smallest that reach the case: one scene trimmed to 1023 / 1024 / 1025 / 2049 kept Gaussians; a chunk boundary on a
bucket's first rank and strictly inside a bucket; a bucket that spans several boundaries in each of the finish kernel's two
exchange forms; runs of empty buckets and a single used bucket; an oversized bucket and a key outside the window (both rendered
again); 1, 64 and a ragged number of tile rows; every Gaussian kept; a grid just over 64 tiles wide, which keeps the old kernels."""
import math

import numpy as np
import pytest
import torch

from _util import scene_inputs, run_native, run_oracle, assert_blend_matches, depth_keys, msd_window, msd_bucket_sizes

pytestmark = pytest.mark.gpu

CHUNK, XCAP, CAP = 1024, 8000, 12288          # RB_CHUNK, MSD_XCAP, GGD_MSD_CAP
ATTRS = ("means3D", "opacities", "shs", "scales", "rotations")


# ---- CPU side: scenes and their premises ---------------------------------------------------------------------------------
def layout(o, window=None):
    """(bucket sizes, first depth rank of every bucket, kept count) of the oracle frame `o` over `window` (default: its own)"""
    sizes = msd_bucket_sizes(o, window)
    assert sizes is not None
    return sizes, np.concatenate([[0], np.cumsum(sizes)[:-1]]), int(sizes.sum())


def bucket_of_rank(sizes, bases, r):
    return int(np.searchsorted(bases + sizes, r, side="right"))


def boundaries_inside(sizes, bases, b):
    """chunk boundaries 1024 k with base <= 1024 k < base + size of bucket b"""
    lo, hi = int(bases[b]), int(bases[b] + sizes[b])
    return [k * CHUNK for k in range((lo + CHUNK - 1) // CHUNK, (hi + CHUNK - 1) // CHUNK) if lo <= k * CHUNK < hi]


def on_screen_scene(P, size, seed, lsm=-5.5, **kw):
    """a cube scene shrunk so that every Gaussian is on screen"""
    d = scene_inputs(P=P, size=size, lsm=lsm, seed=seed, **kw)
    d["means3D"] = (0.3 * d["means3D"]).contiguous()
    return d


def trimmed(d, P):
    t = dict(d, P=P)
    for k in ATTRS:
        t[k] = d[k][:P].contiguous()
    return t


def scene_with_kept_count(N):
    full = on_screen_scene(2600, 128, seed=11)
    vis = np.nonzero(run_oracle(full)["radii"] > 0)[0]
    assert len(vis) >= N
    d = trimmed(full, int(vis[N - 1]) + 1)
    o = run_oracle(d)
    assert int((o["radii"] > 0).sum()) == N                                   # the premise
    return d, o


def boundary_scenes():
    """(scene whose rank 1024 lies strictly inside a bucket, the same scene with later Gaussians replaced by copies of an early one
    until that bucket STARTS at rank 1024), with their oracle frames"""
    d = on_screen_scene(5000, 128, seed=12)
    o = run_oracle(d)
    vis, dk = np.nonzero(o["radii"] > 0)[0], depth_keys(o)
    win = msd_window([(dk.min(), dk.max())])
    sizes, bases, n = layout(o)
    b = bucket_of_rank(sizes, bases, CHUNK)
    assert bases[b] < CHUNK < bases[b] + sizes[b] and n > 2 * CHUNK               # the premise of the "inside" case
    bk = np.minimum((dk - win[0]) >> win[1], 1023)
    need = int(CHUNK - bases[b])
    src = int(vis[np.nonzero(bk < b)[0][0]])
    victims = [int(v) for v, kb, k in zip(vis, bk, dk) if kb > b and k != dk.max()][:need]
    assert len(victims) == need
    e = dict(d)
    for k in ATTRS:
        t = d[k].clone(); t[victims] = d[k][src]; e[k] = t.contiguous()
    oe = run_oracle(e)
    dke = depth_keys(oe)
    assert msd_window([(dke.min(), dke.max())]) == win
    se, be, ne = layout(oe)
    assert ne == n and be[b] == CHUNK and se[b] > 0 and se[:b].sum() == CHUNK    # the premise: bucket b starts on the boundary
    return (d, o), (e, oe)


def dense_scene(squeeze):
    """test_two_launch_sort_with_dense_buckets' scenes (tests/test_raster_gpu.py)"""
    d = scene_inputs(P=60000, size=256, lsm=-5.5, seed=43)
    view = d["viewmatrix"]
    fwd, cam_pos = view[:3, 2], torch.inverse(view)[3, :3]
    m = d["means3D"].clone()
    rel = m[:40000] - cam_pos
    m[:40000] = m[:40000] - (rel @ fwd - 2.7)[:, None] * fwd[None, :] * (1.0 - squeeze)
    d["means3D"] = m.contiguous()
    return d, run_oracle(d)


def gap_scene():
    d = on_screen_scene(6000, 128, seed=13)
    fwd = d["viewmatrix"][:3, 2]
    m = d["means3D"].clone(); m[::2] += 0.6 * fwd
    d["means3D"] = m.contiguous()
    o = run_oracle(d)
    sizes, bases, n = layout(o)
    used = np.nonzero(sizes)[0]
    assert n > 2 * CHUNK and np.diff(used).max() > 10 and (sizes == 0).sum() > 100   # the premise: a run of empty buckets between used ones
    return d, o


def duplicates_scene(P, size, seed, first, count, opacity):
    """`count` exact copies of one visible Gaussian from index `first` on (equal keys: one bucket whatever the window)"""
    d = scene_inputs(P=P, size=size, lsm=-5.5, seed=seed)
    src = int(np.nonzero(run_oracle(d)["radii"] > 0)[0][0])
    for k in ATTRS:
        t = d[k].clone(); t[first:first + count] = t[src]; d[k] = t.contiguous()
    d["opacities"] = (d["opacities"] * opacity).contiguous()
    return d, run_oracle(d)


# ---- GPU side ------------------------------------------------------------------------------------------------------------
def _ctx():
    from gaussian_gan_decoder_amd import _capi
    return _capi, _capi.context_for(torch.device("cuda:0"))


def _stats(ctx, _capi):
    return tuple(ctx.get_option(s) for s in (_capi.STAT_MSD_FRAMES, _capi.STAT_SORT_RERUNS, _capi.STAT_L1_COUNTED_FRAMES))


def _frame(d, o, what):
    n = run_native(d, debug=False)
    assert n["num_rendered"] == o["num_rendered"], what
    np.testing.assert_array_equal(n["point_list"], o["point_list"], err_msg=str(what))
    np.testing.assert_array_equal(n["ranges"], o["ranges"], err_msg=str(what))
    return n


def _until_two_launches(d, o, counted, takes_counted=True):
    """arm the two-launch sort and render `d` until three frames have run it; returns the last frame"""
    _capi, ctx = _ctx()
    ctx.set_option(_capi.OPT_L1_COUNTED, counted)
    ctx.set_option(_capi.OPT_MSD_SORT, 1)                   # (restarts the speculation state: this scene's window)
    m0, r0, c0 = _stats(ctx, _capi)
    for i in range(40):
        n = _frame(d, o, (counted, i))
        if ctx.get_option(_capi.STAT_MSD_FRAMES) >= m0 + 3:
            break
    m1, r1, c1 = _stats(ctx, _capi)
    assert m1 == m0 + 3 and i >= 8, "the two-launch sort never ran"
    assert r1 == r0, "a frame was rendered again"
    assert c1 - c0 == (3 if counted and takes_counted else 0)
    return n


def _same_binning(a, b):
    R = a["num_rendered"]
    assert R == b["num_rendered"] and torch.equal(a["binning"][:4 * R], b["binning"][:4 * R])
    np.testing.assert_array_equal(a["ranges"], b["ranges"])


def _both_kernels(d, o, takes_counted=True):
    _capi, ctx = _ctx()
    assert ctx.get_option(_capi.OPT_L1_COUNTED) == 1, "the counted level 1 is the default"
    try:
        n1 = _until_two_launches(d, o, 1, takes_counted)
        assert_blend_matches(n1, o)
        n0 = _until_two_launches(d, o, 0)
        _same_binning(n1, n0)
    finally:
        ctx.set_option(_capi.OPT_L1_COUNTED, 1)
    return n1


@pytest.mark.parametrize("N", [1023, 1024, 1025, 2049])
def test_kept_counts_around_one_chunk(native_lib, N):
    """1023 / 1024 kept Gaussians: one chunk, no boundary below the kept count; 1025: a second chunk of one item; 2049: a third"""
    _both_kernels(*scene_with_kept_count(N))


@pytest.mark.parametrize("which", [0, 1], ids=["inside-a-bucket", "on-a-bucket-start"])
def test_chunk_boundary_inside_a_bucket_and_on_its_first_rank(native_lib, which):
    _both_kernels(*boundary_scenes()[which])


@pytest.mark.parametrize("squeeze,lo,hi", [(0.008, 6000, XCAP), (0.002, XCAP, CAP)], ids=["lds-exchange", "global-exchange"])
def test_one_bucket_spans_several_chunk_boundaries(native_lib, squeeze, lo, hi):
    d, o = dense_scene(squeeze)
    sizes, bases, n = layout(o)
    b = int(sizes.argmax())
    assert lo < sizes[b] <= hi and len(boundaries_inside(sizes, bases, b)) >= 3, (sizes[b], bases[b])   # the premise
    _both_kernels(d, o)


def test_runs_of_empty_buckets(native_lib):
    _both_kernels(*gap_scene())


def test_every_key_in_one_bucket(native_lib):
    d, o = duplicates_scene(2000, 128, seed=14, first=0, count=2000, opacity=0.02)
    sizes, bases, n = layout(o)
    assert n == 2000 and (sizes > 0).sum() == 1                                 # the premise
    _both_kernels(d, o)


def _armed(counted):
    _capi, ctx = _ctx()
    ctx.set_option(_capi.OPT_L1_COUNTED, counted)
    ctx.set_option(_capi.OPT_MSD_SORT, 1)                   # (restarts the speculation state)
    return _capi, ctx, _stats(ctx, _capi)


def _oversized_frames(d, o, counted):
    """fourteen frames, as test_two_launch_sort_with_more_equal_keys_than_a_bucket_holds: the first speculated one fails its check"""
    _capi, ctx, (m0, r0, c0) = _armed(counted)
    for i in range(14):
        n = _frame(d, o, (counted, i))
    m1, r1, c1 = _stats(ctx, _capi)
    assert m1 == m0 and r1 == r0 + 1
    assert c1 - c0 == (1 if counted else 0)      # (the failed frame's binning ran once, on the counted tables)
    return n


def test_an_oversized_bucket_is_rendered_again(native_lib):
    """14 000 equal keys (test_two_launch_sort_with_more_equal_keys_than_a_bucket_holds' scene): the first speculated frame fails its
    own check after the finish kernel counted the bucket's rows window by window, and is rendered again by the ordinary path"""
    d, o = duplicates_scene(40000, 192, seed=47, first=20000, count=14000, opacity=0.02)
    assert layout(o)[0].max() > CAP                                              # the premise
    _capi, ctx = _ctx()
    try:
        n1 = _oversized_frames(d, o, 1)
        assert_blend_matches(n1, o)
        _same_binning(n1, _oversized_frames(d, o, 0))
    finally:
        ctx.set_option(_capi.OPT_L1_COUNTED, 1)


def _pose_change(a, oa, b, ob, counted):
    n = _until_two_launches(a, oa, counted)      # the window holds pose a's keys
    _capi, ctx = _ctx()
    m0, r0, c0 = _stats(ctx, _capi)
    n = _frame(b, ob, (counted, "pose b"))
    m1, r1, c1 = _stats(ctx, _capi)
    assert m1 == m0 and r1 == r0 + 1, "the frame with a key outside the window was not rendered again"
    assert c1 - c0 == (1 if counted else 0)
    return n


def test_a_key_outside_the_window_is_rendered_again(native_lib):
    """a pose change once the window has formed: the oblique view's near corner lies below the head-on window"""
    a = scene_inputs(P=20000, size=128, lsm=-5.0, seed=81)
    b = scene_inputs(P=20000, size=128, lsm=-5.0, seed=81, h=math.pi / 2 + 0.95, v=math.pi / 2 - 0.28)
    oa, ob = run_oracle(a), run_oracle(b)
    ka, kb = depth_keys(oa), depth_keys(ob)
    lo, sh = msd_window([(ka.min(), ka.max())])
    assert kb.min() < lo or ((kb.max() - lo) >> sh) > 1023                      # the premise
    assert len(kb) > CHUNK
    _capi, ctx = _ctx()
    try:
        n1 = _pose_change(a, oa, b, ob, 1)
        assert_blend_matches(n1, ob)
        _same_binning(n1, _pose_change(a, oa, b, ob, 0))
    finally:
        ctx.set_option(_capi.OPT_L1_COUNTED, 1)


@pytest.mark.parametrize("W,H,P", [(256, 16, 20000), (64, 1024, 6000), (200, 100, 8000)], ids=["1-tile-row", "64-tile-rows", "ragged-rows"])
def test_tile_row_counts(native_lib, W, H, P):
    d = scene_inputs(P=P, size=max(W, H), seed=15, lsm=-4.5, width=W, height=H)
    o = run_oracle(d)
    assert layout(o)[2] > CHUNK                                                  # the premise: at least one chunk boundary
    _both_kernels(d, o)


def test_every_gaussian_kept(native_lib):
    """test_two_launch_sort_when_every_key_of_a_sort_tile_is_kept's scene: all 4096 keys of a sort tile are kept"""
    d = on_screen_scene(30000, 256, seed=61)
    view = d["viewmatrix"]
    by_depth = torch.argsort(d["means3D"] @ view[:3, 2] + view[3, 2])
    for k in ATTRS:
        d[k] = d[k][by_depth].contiguous()
    o = run_oracle(d)
    assert (o["radii"] > 0).all()                                                # the premise
    _both_kernels(d, o)


def test_a_wide_grid_keeps_the_old_kernels(native_lib):
    """65 x 4 tiles: the wide row binning; the counter stands still and the lists equal the oracle's"""
    d = scene_inputs(P=6000, size=1040, seed=16, lsm=-4.5, width=1040, height=64)
    o = run_oracle(d)
    assert layout(o)[2] > CHUNK
    _both_kernels(d, o, takes_counted=False)
