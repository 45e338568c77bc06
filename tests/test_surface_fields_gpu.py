"""GPU iso-surface point sampler (csrc/ggd_surface.hip) with EVERY output point checked, on rough, tied, steep and open fields.

test_surface_sampler.py compares some 300 of 500 000 points with the restatement, on smooth closed fields at n >= 64.  Here every
point of every call is held to two references (test_surface_fields_host.py checks the references themselves without a GPU):
  restatement  point i == ((w0 v0 + w1 v1) + w2 v2) / n - 0.5 on _surface_ref.numbered_faces[i mod F], within 2e-6 absolute (the
               bar test_surface_sampler.py uses for the same expression), and num_faces == F;
  interpolant  |kuhn_interpolant(point)| <= K 2^-24 n D, D the largest |sigma - level| over the corners of the point's cell: the
               point lies on the zero set of the float64 piecewise-linear interpolant, which knows nothing of the kernel's case
               split, edge order or numbering.  K = 30.24 = 4 x 7.56: the float32 restatement's own points, pushed through the
               same / n - 0.5 transform, reach 7.554 over all the fields below (measured on the host, and measured again by
               test_surface_fields_host.py::test_interpolant_bound_is_four_times_the_float32_twin); the factor 4 covers FMA
               contraction and another order of the three products, which move a point by ulps of its coordinate, not by a cell.
               No point is excluded.  On the MI355X the kernel's points reach 4.86 (rough fields), 2.86 (sphere, n = 82), and
               differ from the restatement by at most 2.4e-7.

Grids (cells = (n - 1)^3 feed the stand-alone prefix scan: 2048-element tiles, 8 items per thread):
  n = 2   1 cell        one partial scan thread            one_corner(0..7), empty, full
  n = 3   8 cells       exactly one thread's 8 items       the same
  n = 9   512           all 16 patterns of every tetrahedron     noise, ties, steep, open
  n = 14  2197          two tiles, ragged tail (2197 mod 8 = 5)  the same
  n = 17  4096          exactly two full tiles                   the same
  n = 18  4913          all 256 cell patterns, ragged third tile the same
  n = 82  531 441       260 block sums: the second round of the block-sum scan    sphere
num_points in {F // 2, F - 1, F, F + 1, 2 F + 3} (n = 82: F + 1), seeds 77 and 2^64 - 1 in turn; num_points < F gives the first
num_points faces, as the reference truncates after its first pass (target_dataloader.py:108-114).

Thickness clip (noise, n = 9, N = 4 F = 12176, surface_thickness = 5): points with 1 + 5 g within 1e-3 of 0 or of 1 are left out,
0.033 % .. 0.057 % of the points for the seeds 0, 77, 2^32, 2^64 - 1 of the restated generator (4 .. 7 points; the bar is 0.1 %);
some 42 % are clipped to the origin, 50 % kept as they are, 8 % scaled.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _surface_ref as SR
from test_surface_sampler import _field as analytic_field

pytestmark = pytest.mark.gpu

LEVEL = 10.0
K = SR.K_INTERPOLANT
SEED_A, SEED_B = 77, 2 ** 64 - 1
FIELDS = dict(SR.small_fields())
ROUGH_IDS = [f"{name}-{n}" for name in SR.ROUGH for n in SR.ROUGH_SIZES]
CORNER_IDS = [f"one_corner{c}-{n}" for n in (2, 3) for c in range(8)]
FLAT_IDS = [f"{name}-{n}" for name in ("empty", "full") for n in (2, 3)]


@functools.lru_cache(maxsize=None)
def _faces(fid, level=LEVEL, shift=0.0):
    """(field, numbered faces) of a field id, computed once and shared; shift: the field minus a constant (the level tests)."""
    sig = analytic_field("sphere", 82) if fid == "sphere-82" else FIELDS[fid]
    if shift:
        sig = sig - np.float32(shift)
    sig.setflags(write=False)
    faces = SR.numbered_faces(sig, level)
    faces.setflags(write=False)
    return sig, faces


def _sample(sig, level, num_points, thickness, seed):
    from gaussian_gan_decoder_amd.target_sampler import sample_surface_points
    t = sig if torch.is_tensor(sig) else torch.from_numpy(np.array(sig)).to("cuda:0")
    pos, nf = sample_surface_points(t, level=level, num_points=num_points, surface_thickness=thickness, seed=seed)
    assert pos.shape == (num_points, 3) and pos.dtype == torch.float32
    return pos.cpu().numpy(), int(nf.item())


def _check_call(sig, level, faces, num_points, seed):
    """One thickness-0 call: face count, every point against the restatement and against the float64 interpolant."""
    p, nf = _sample(sig, level, num_points, 0.0, seed)
    F = len(faces)
    assert nf == F, (nf, F)
    assert np.isfinite(p).all()
    want = SR.restated_points(sig, level, seed, num_points, faces)
    err = np.abs(p - want).max() if num_points else 0.0
    ratio = SR.interpolant_ratio(sig, level, p).max() if num_points and F else 0.0
    print(f"n = {sig.shape[0]}, F = {F}, N = {num_points}, seed {seed}: |p - restatement| <= {err:.2e}, interpolant ratio <= {ratio:.3f} (K = {K})")
    assert err <= 2e-6, (num_points, seed, int(np.abs(p - want).max(1).argmax()))
    assert ratio <= K, (num_points, seed, int(SR.interpolant_ratio(sig, level, p).argmax()))
    return p


def _counts(F):
    return sorted({max(0, v) for v in (F // 2, F - 1, F, F + 1, 2 * F + 3)})


@pytest.mark.parametrize("fid", ROUGH_IDS + CORNER_IDS)
def test_every_point_against_restatement_and_interpolant(native_lib, fid):
    sig, faces = _faces(fid)
    F = len(faces)
    assert F > 0
    if fid in CORNER_IDS:
        assert F == (6 if fid.startswith(("one_corner0", "one_corner7")) else 2)
    for k, N in enumerate(_counts(F)):
        _check_call(sig, LEVEL, faces, N, (SEED_A, SEED_B)[k % 2])
    _check_call(sig, LEVEL, faces, F + 1, SEED_B)       # (F + 1 with the other seed: the wrap to face 0 under both)


def test_every_point_behind_a_two_round_block_sum_scan(native_lib):
    """531 441 cells = 260 scan tiles: the block sums themselves need a second round of 256."""
    sig, faces = _faces("sphere-82")
    assert (sig.shape[0] - 1) ** 3 > 256 * 2048
    _check_call(sig, LEVEL, faces, len(faces) + 1, SEED_B)


@pytest.mark.parametrize("level", [0.0, -3.0])
def test_other_levels(native_lib, level):
    """noise - 10 at level 0 and noise - 13 at level -3 cut the same cells as noise at level 10."""
    _, faces10 = _faces("noise-9")
    sig, faces = _faces("noise-9", level, LEVEL - level)
    assert len(faces) == len(faces10) > 0
    if level == 0.0:
        assert np.array_equal(faces, faces10)       # (sigma - 10) - 0 is sigma - 10: the very same triangles
    for N, seed in ((len(faces) + 1, SEED_A), (2 * len(faces) + 3, SEED_B)):
        _check_call(sig, level, faces, N, seed)


@pytest.mark.parametrize("seed", [SEED_A, SEED_B])
def test_thickness_clip_at_both_ends(native_lib, seed):
    sig, faces = _faces("noise-9")
    N = 4 * len(faces)
    p0 = _check_call(sig, LEVEL, faces, N, seed)
    pt, nf = _sample(sig, LEVEL, N, 5.0, seed)
    assert nf == len(faces)
    s = 1.0 + 5.0 * SR.point_random_numbers(seed, np.arange(N))[3].astype(np.float64)
    low, high = s <= -1e-3, s >= 1.0 + 1e-3
    mid = (s >= 1e-3) & (s <= 1.0 - 1e-3)
    skipped = 1.0 - (low.sum() + mid.sum() + high.sum()) / N
    print(f"seed {seed}: {low.mean():.3f} clipped to 0, {mid.mean():.3f} scaled, {high.mean():.3f} kept, {100 * skipped:.3f} % left out")
    assert skipped < 1e-3
    assert low.sum() > N // 4 and high.sum() > N // 4 and mid.sum() > N // 40        # each branch is really present
    assert (pt[low] == 0.0).all()
    assert np.array_equal(pt[high].view(np.uint32), p0[high].view(np.uint32))
    ratio = np.linalg.norm(pt[mid].astype(np.float64), axis=1) / np.maximum(np.linalg.norm(p0[mid].astype(np.float64), axis=1), 1e-9)
    assert np.abs(ratio - s[mid]).max() <= 1e-4, float(np.abs(ratio - s[mid]).max())


@pytest.mark.parametrize("fid", FLAT_IDS)
def test_fields_without_a_surface(native_lib, fid):
    sig, faces = _faces(fid)
    assert len(faces) == 0
    for N in (0, 1, 5):
        p, nf = _sample(sig, LEVEL, N, 0.0, SEED_A)
        assert nf == 0 and p.shape == (N, 3) and (p == 0.0).all()


@pytest.mark.parametrize("fid", ["noise-9", "one_corner3-2", "one_corner7-3"])
def test_no_point_and_one_point(native_lib, fid):
    sig, faces = _faces(fid)
    p, nf = _sample(sig, LEVEL, 0, 0.0, SEED_A)
    assert p.shape == (0, 3) and nf == len(faces) > 0
    for seed in (SEED_A, SEED_B):
        _check_call(sig, LEVEL, faces, 1, seed)


def test_inputs_as_callers_pass_them(native_lib):
    from gaussian_gan_decoder_amd.target_sampler import sample_surface_points
    dev = torch.device("cuda:0")
    sig, _ = _faces("noise-14")
    base = torch.from_numpy(np.array(sig)).to(dev)
    view = base.permute(2, 0, 1)                                  # a transposed, non-contiguous view of the cube
    assert not view.is_contiguous()
    sig_t = np.ascontiguousarray(np.transpose(sig, (2, 0, 1)))
    faces_t = SR.numbered_faces(sig_t, LEVEL)
    N = len(faces_t) + 7
    args = dict(level=LEVEL, num_points=N, surface_thickness=0.3, seed=SEED_B)
    a, nfa = sample_surface_points(view, **args)
    b, nfb = sample_surface_points(view.contiguous(), **args)
    c, nfc = sample_surface_points(view.contiguous(), **args)     # the same arguments again
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        d, nfd = sample_surface_points(view, **args)
    side.synchronize()
    torch.cuda.synchronize(dev)
    assert int(nfa.item()) == int(nfb.item()) == int(nfc.item()) == int(nfd.item()) == len(faces_t)
    for other in (b, c, d):
        assert torch.equal(a.view(torch.int32), other.view(torch.int32))
    _check_call(sig_t, LEVEL, faces_t, N, SEED_B)                 # and the view is read as the transposed cube


# ------------------------------------------------------------------------------------------------- refusals -----
REFUSALS = [
    # (what, n, num_points, tmp_bytes: None = what ggd_surface_tmp_bytes(9) asks for, message)
    ("n = 712: 12 * 711^3 faces do not fit uint32", 712, 4, 1, "bad grid size"),
    ("n = 1024", 1024, 4, 1, "bad grid size"),
    ("n = 1", 1, 4, None, "bad grid size"),
    ("n = 0", 0, 4, None, "bad grid size"),
    ("num_points = -1", 9, -1, None, "bad grid size / point count"),
    ("tmp one byte short", 9, 4, -1, "tmp too small"),
    ("tmp_bytes = 0", 9, 4, 0, "tmp too small"),
]


@pytest.mark.parametrize("row", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_launch_nothing(native_lib, row):
    """ggd_surface_sample through ctypes, as test_capi_refusals_gpu.py does for the rasterizer: each call returns from validation
    with the message, and positions / num_faces keep their sentinels.  (n = 712 and 1024 are passed with tmp_bytes = 1, so that
    nothing could be launched on a 9^3 buffer whatever the order of the checks; the message says which check refused.)"""
    from gaussian_gan_decoder_amd import _capi
    _, n, num_points, tmp_bytes, msg = row
    dev = torch.device("cuda:0")
    ctx, stream = _capi.context_and_stream(dev)
    lib = ctx.lib
    need = lib.ggd_surface_tmp_bytes(9)
    assert need > 0 and lib.ggd_surface_tmp_bytes(711) > need
    assert lib.ggd_surface_tmp_bytes(712) == 0 and lib.ggd_surface_tmp_bytes(1) == 0 and lib.ggd_surface_tmp_bytes(2) > 0
    sig, faces = _faces("noise-9")
    sigma = torch.from_numpy(np.array(sig)).to(dev)
    tmp = torch.zeros((need,), dtype=torch.uint8, device=dev)
    pos = torch.full((4, 3), 7.0, dtype=torch.float32, device=dev)
    nf = torch.full((1,), 12345, dtype=torch.int32, device=dev)
    tb = need if tmp_bytes is None else (need - 1 if tmp_bytes < 0 else tmp_bytes)
    rc = lib.ggd_surface_sample(ctx.handle, C.c_void_p(stream), C.c_void_p(sigma.data_ptr()), n, LEVEL, num_points, 0.0,
                                C.c_uint64(SEED_A), C.c_void_p(pos.data_ptr()), C.c_void_p(nf.data_ptr()), C.c_void_p(tmp.data_ptr()), tb)
    err = lib.ggd_last_error(ctx.handle).decode()
    torch.cuda.synchronize(dev)
    assert rc == -1 and msg in err, (row, rc, err)
    assert (pos == 7.0).all() and int(nf.item()) == 12345 and int(tmp.max()) == 0
    # the context is still usable: the same buffers, asked properly
    rc = lib.ggd_surface_sample(ctx.handle, C.c_void_p(stream), C.c_void_p(sigma.data_ptr()), 9, LEVEL, 4, 0.0, C.c_uint64(SEED_A),
                                C.c_void_p(pos.data_ptr()), C.c_void_p(nf.data_ptr()), C.c_void_p(tmp.data_ptr()), need)
    torch.cuda.synchronize(dev)
    assert rc == 0 and int(nf.item()) == len(faces)
    assert np.abs(pos.cpu().numpy() - SR.restated_points(sig, LEVEL, SEED_A, 4, faces)).max() <= 2e-6
