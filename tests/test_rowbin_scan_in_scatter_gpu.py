"""Row binning without its level-2 scan launch (rb_scatter2_kernel<true>, ggd_rowbin.hip): on the single-call folded path the
per-Gaussian kernel counts the instances per tile row and every level-2 scatter workgroup forms its tile starts from the raw
count rows of its tile row's blocks.  Every case renders a frame in the exact form first (a shape without a capacity hint takes
the two-call form; or GGD_OPT_FOLD = 0: both run rb_scan2_kernel) and then on the folded path, and compares num_rendered, the
sorted list, the ranges of EVERY tile, image, final_T, n_contrib and radii bit for bit.  GGD_STAT_SCAN_IN_SCATTER_FRAMES says
that the new kernel ran (and that the exact form did not use it).

Shapes: the smallest at which the kernel can go wrong -- block edges of the 1024-entry level-2 chunks inside one tile (every
other tile row empty: their zero ranges come from workgroups of other rows), one tile row of about 40 blocks over all columns (two
load batches of 4 waves x 8 rows, all four waves), the same on a 17-column grid, 1 x 1 and 64 x 1 grids, partial edge tiles, a
shell, a capacity overflow with its retry, and two scenes in alternation (each frame's row totals come from its own block)."""
import numpy as np
import pytest
import torch

from _util import scene_inputs, run_native

pytestmark = pytest.mark.gpu


def _ctx():
    from gaussian_gan_decoder_amd import _capi
    return _capi, _capi.context_for(torch.device("cuda:0"))


def _ran(ctx, _capi):
    return ctx.get_option(_capi.STAT_SCAN_IN_SCATTER_FRAMES)


def _assert_same_frame(n, e, what):
    R = e["num_rendered"]
    assert n["num_rendered"] == R, what
    np.testing.assert_array_equal(n["point_list"][:R], e["point_list"][:R], err_msg=what)
    np.testing.assert_array_equal(n["ranges"], e["ranges"], err_msg=what)
    assert torch.equal(n["color"], e["color"]), what
    np.testing.assert_array_equal(n["final_T"], e["final_T"], err_msg=what)
    np.testing.assert_array_equal(n["n_contrib"], e["n_contrib"], err_msg=what)
    assert torch.equal(n["radii"], e["radii"]), what


def _exact_then_folded(d, frames=1):
    """The frame in the two-call form (no hint for the shape), then `frames` times on the single-call folded path."""
    _capi, ctx = _ctx()
    assert ctx.get_option(_capi.OPT_FOLD) == 1
    ctx.capacity_hint.pop((d["P"], d["W"], d["H"]), None)
    c0 = _ran(ctx, _capi)
    exact = run_native(d, debug=False)
    assert _ran(ctx, _capi) == c0, "the exact form must run the scan kernel"
    for f in range(frames):
        n = run_native(d, debug=False)
        assert _ran(ctx, _capi) == c0 + f + 1, "the scan-in-scatter kernel did not run"
        _assert_same_frame(n, exact, f"frame {f}")
    return exact


def _placed(P, W, H, px, py, seed):
    """P tiny splats (radius 2 px: only the 0.3 px^2 dilation remains) whose centres project to the pixels (px, py), at
    slightly different depths."""
    d = scene_inputs(P=P, size=max(W, H), lsm=-6.0, seed=seed, width=W, height=H)
    view, proj = d["viewmatrix"].double(), d["projmatrix"].double()
    cam = torch.inverse(view)[3, :3]
    u, v, fwd = view[:3, 0], view[:3, 1], view[:3, 2]

    def ndc(p):
        h = torch.cat([p, torch.ones(1, dtype=torch.float64)]) @ proj
        return h[:2] / h[3]

    c1 = cam + fwd                                    # at unit depth ndc is affine in the offsets along u and v
    n0 = ndc(c1)
    G = torch.stack([ndc(c1 + u) - n0, ndc(c1 + v) - n0], dim=1)      # d ndc / d (a, b)
    g = torch.Generator().manual_seed(seed + 7)
    z = 2.5 + 0.5 * torch.rand(P, generator=g, dtype=torch.float64)
    want = torch.stack([(2.0 * torch.as_tensor(px, dtype=torch.float64) + 1.0) / W - 1.0,
                        (2.0 * torch.as_tensor(py, dtype=torch.float64) + 1.0) / H - 1.0], dim=1)
    ab = torch.linalg.solve(G, (want - n0).T).T       # offsets at unit depth
    xyz = cam + z[:, None] * (fwd + ab[:, :1] * u + ab[:, 1:] * v)
    d["means3D"] = xyz.float().contiguous()
    d["scales"] = torch.full((P, 3), 1e-6)
    return d


@pytest.mark.parametrize("N", [1023, 1024, 1025, 2049])
def test_equal_splats_in_one_tile_at_chunk_edges(native_lib, N):
    """N splats at one pixel of tile (31, 18) of a 64 x 64 grid: 1, 1, 2 and 3 level-2 blocks in tile row 18 (a full last chunk, a
    one-entry last chunk), nothing in the other 63 rows."""
    d = _placed(N, 1024, 1024, np.full(N, 31 * 16 + 8.0), np.full(N, 18 * 16 + 8.0), seed=N)
    e = _exact_then_folded(d)
    assert e["num_rendered"] == N
    lens = (e["ranges"][:, 1] - e["ranges"][:, 0]).reshape(64, 64)
    assert lens[18, 31] == N and lens.sum() == N
    assert (e["ranges"].reshape(64, 64, 2)[np.arange(64) != 18] == 0).all()


@pytest.mark.parametrize("W,H,row", [(1024, 1024, 41), (272, 64, 2)], ids=["64-columns", "17-columns"])
def test_forty_blocks_in_one_tile_row(native_lib, W, H, row):
    """40 460 entries in ONE tile row, over all columns: 40 blocks (the last one ragged) -- two load batches per wave, all four waves,
    `before` of every chunk position."""
    P = 40 * 1024 - 500
    g = torch.Generator().manual_seed(W)
    px = (2.5 + (W - 5.0) * torch.rand(P, generator=g, dtype=torch.float64)).numpy()
    py = (row * 16 + 3.0 + 10.0 * torch.rand(P, generator=g, dtype=torch.float64)).numpy()
    d = _placed(P, W, H, px, py, seed=W + 1)
    e = _exact_then_folded(d)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r = e["rect"]
    assert (r[:, 1] == row).all() and (r[:, 3] == row + 1).all(), "every splat lies in the one tile row"
    lens = (e["ranges"][:, 1] - e["ranges"][:, 0]).reshape(gy, gx)
    assert (lens[row] > 0).all() and lens.sum() == lens[row].sum() == e["num_rendered"] > P


@pytest.mark.parametrize("case", [
    dict(P=3000, size=16, lsm=-4.0),                                   # 1 x 1 tiles
    dict(P=20000, size=1024, lsm=-5.0, width=1024, height=16),         # 64 x 1 tiles
    dict(P=50000, size=1000, lsm=-5.5),                                # 63 x 63 tiles, partial edge tiles
    dict(P=100000, size=512, kind="shell", lsm=-5.5),
], ids=["1x1", "64x1", "1000x1000", "shell-512"])
def test_grids_and_a_shell(native_lib, case):
    e = _exact_then_folded(scene_inputs(seed=21, **case), frames=2)
    assert e["num_rendered"] > 0


def test_capacity_overflow_is_retried_and_the_next_frame_is_exact(native_lib):
    """A small scene sets the capacity hint; a scene of the same shape with about 4 x the instances overflows it on the folded path
    (the scatter then works on clamped rows and row totals that do not match them: every store stays behind the capacity
    guard) and is rendered again; that frame and the next folded one equal the exact form."""
    from gaussian_gan_decoder_amd.rasterizer import _capacity
    _capi, ctx = _ctx()
    P, S = 60000, 256
    small = scene_inputs(P=P, size=S, lsm=-6.5, seed=31)
    big = scene_inputs(P=P, size=S, lsm=-4.9, seed=31)
    ctx.capacity_hint.pop((P, S, S), None)
    n_small = run_native(small, debug=False)                      # two-call form, records the hint
    c0 = _ran(ctx, _capi)
    _assert_same_frame(run_native(small, debug=False), n_small, "small, folded")
    assert _ran(ctx, _capi) == c0 + 1
    retries = ctx.capacity_retries
    n_big = run_native(big, debug=False)                          # folded, overflows, rendered again with an exact buffer
    assert ctx.capacity_retries == retries + 1
    assert n_big["num_rendered"] > _capacity(n_small["num_rendered"])
    assert 3 * n_small["num_rendered"] < n_big["num_rendered"] < 6 * n_small["num_rendered"]
    saved = ctx.get_option(_capi.OPT_FOLD)
    try:
        ctx.set_option(_capi.OPT_FOLD, 0)
        c1 = _ran(ctx, _capi)
        exact = run_native(big, debug=False)                      # single call, separate histogram launch, rb_scan2_kernel
        assert _ran(ctx, _capi) == c1
    finally:
        ctx.set_option(_capi.OPT_FOLD, saved)
    _assert_same_frame(n_big, exact, "big, retried")
    n_big2 = run_native(big, debug=False)                         # the hint fits now
    assert ctx.capacity_retries == retries + 1 and _ran(ctx, _capi) == c1 + 1
    _assert_same_frame(n_big2, exact, "big, folded")


def test_two_scenes_in_alternation(native_lib):
    """Six folded frames, two scenes of one shape in turn: each frame's instances per row are accumulated in the block the frame
    before cleared -- a total left over from the other scene would shift every tile start behind it."""
    _capi, ctx = _ctx()
    P, S = 30011, 256
    scenes = [scene_inputs(P=P, size=S, lsm=-5.0, seed=41), scene_inputs(P=P, size=S, kind="shell", lsm=-4.6, seed=42)]
    saved = ctx.get_option(_capi.OPT_FOLD)
    try:
        ctx.set_option(_capi.OPT_FOLD, 0)
        ctx.capacity_hint.pop((P, S, S), None)
        exact = [run_native(d, debug=False) for d in (scenes[1], scenes[0])][::-1]
    finally:
        ctx.set_option(_capi.OPT_FOLD, saved)
    assert exact[0]["num_rendered"] != exact[1]["num_rendered"]
    c0 = _ran(ctx, _capi)
    for f in range(6):
        n = run_native(scenes[f % 2], debug=False)
        _assert_same_frame(n, exact[f % 2], f"frame {f}")
    assert _ran(ctx, _capi) == c0 + 6
