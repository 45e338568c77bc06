"""The references of the surface-sampler GPU tests (test_surface_fields_gpu.py), checked on the host: no GPU needed.

`_surface_ref.face_triangle` / `numbered_faces` restate the kernel (csrc/ggd_surface.hip) and so pin the implementation, not the
operation.  What says that the emitted triangles ARE the iso-surface is independent of the kernel's case split:
  * `kuhn_interpolant`: the float64 piecewise-linear interpolant of sigma - level on the six tetrahedra around each cell's 0-7
    diagonal, written without a case table.  The iso-surface is its zero set;
  * `edge_uses`: a closed surface uses every edge an even number of times (exactly twice where no vertex sits on a grid corner),
    an open one has its odd edges on the boundary of the grid.
Both are held against the restated triangles here, on fields that are rough (uniform noise), tied (integer values, many corners
exactly at the level), steep (0 / 3e4) and open (noise up to the grid boundary), at the sizes the GPU tests run.

Measured with the committed seed (FIELD_SEED, level 10):
  pattern coverage   noise, n = 18: 256 of 256 corner sign patterns of a cell (the rarest 6 times); n = 9, 14, 17, 18: 16 of 16
                     patterns of each of the six tetrahedra, and cells with 12 faces at every size
  watertight         noise / steep, n = 9 / 14 / 17 / 18: 4566 / 21948 / 41538 / 50430 and 4410 / 21756 / 41640 / 50148 edges, all
                     used twice; ties: 3359 / 16361 / 30678 / 36836 edges used 2 .. 24 times, none odd, with 498 / 2090 / 4690 /
                     5952 triangles collapsed onto a corner; open: 572 / 1462 / 2326 / 2552 odd edges, all on the grid boundary
  generator          2^18 indices, seeds 0 / 77 / 2^32 / 2^64 - 1: |mean - 1/3| <= 6e-4 against a bar of 5 standard errors =
                     1.75e-3 (sd 0.179); |lag-1 correlation of w0|, |correlation of w0 and the thickness draw| <= 2.9e-3 against
                     5 / sqrt(N) = 9.8e-3
  interpolant        at the float64 vertices of all_triangles(corner_dtype=float64): <= 1.7e-15 of the field's range, bar 1e-9
                     (with the kernel's float32 corner differences the noise fields give 1.3e-8: the rounding of sigma - 10)
  float32 twin       largest |interpolant| / (2^-24 n D) of the restatement's own float32 points: 7.554 (noise, n = 18; rough
                     fields 3.3 .. 7.6, sphere at n = 82 5.2, single cells 1 .. 3) -> _surface_ref.K_MEASURED = 7.56, K = 30.24
"""
import numpy as np
import pytest

import _surface_ref as SR
from test_surface_sampler import _field as analytic_field

LEVEL = 10.0
SEEDS = (0, 77, 2 ** 32, 2 ** 64 - 1)
FIELDS = dict(SR.small_fields())
FIELDS["sphere-82"] = analytic_field("sphere", 82)
CLOSED = [f"{name}-{n}" for name in ("noise", "ties", "steep") for n in SR.ROUGH_SIZES]


@pytest.mark.parametrize("fid", list(FIELDS))
def test_numbered_faces_equal_face_triangle_at_every_face(fid):
    sig = FIELDS[fid]
    cnt = SR.cell_face_counts(sig, LEVEL)
    off = np.cumsum(cnt)
    faces = SR.numbered_faces(sig, LEVEL)
    assert faces.dtype == np.float32 and faces.shape == (int(cnt.sum()), 3, 3)
    for i in range(len(faces)):
        want = SR.face_triangle(sig, LEVEL, off, i)
        assert want.dtype == np.float32
        assert np.array_equal(faces[i].view(np.uint32), want.view(np.uint32)), (fid, i, faces[i], want)


@pytest.mark.parametrize("fid", CLOSED)
def test_closed_fields_are_watertight(fid):
    sig = FIELDS[fid]
    edges, uses, collapsed = SR.edge_uses(sig, LEVEL)
    F = int(SR.cell_face_counts(sig, LEVEL).sum())
    print(f"{fid}: {F} faces, {len(uses)} edges, uses {np.unique(uses).tolist()}, {collapsed} collapsed triangles")
    assert len(uses) > 0
    assert (uses % 2 == 0).all(), (fid, int((uses % 2 == 1).sum()))
    if fid.startswith("ties"):
        assert collapsed > 0                      # the case is really present: vertices that sit on a corner at the level
        assert (sig == LEVEL).sum() > sig.size // 10
    else:
        assert (uses == 2).all() and collapsed == 0
        assert 2 * len(uses) == 3 * F             # a closed triangle surface: 3 F / 2 edges


@pytest.mark.parametrize("n", SR.ROUGH_SIZES)
def test_open_field_has_its_odd_edges_on_the_grid_boundary(n):
    sig = FIELDS[f"open-{n}"]
    edges, uses, _ = SR.edge_uses(sig, LEVEL)
    odd = edges[uses % 2 == 1]                                             # [E, 2 vertices, 2 corners] global corner ids
    print(f"open-{n}: {len(odd)} odd edges of {len(uses)}")
    assert len(odd) > 0                                                    # the surface does leave the grid
    xyz = np.stack([odd // (n * n), (odd // n) % n, odd % n], -1)          # [E, 2, 2, 3]
    # a vertex lies on a boundary face when both corners of its grid edge share a coordinate that is 0 or n - 1
    on_face = ((xyz[:, :, 0, :] == xyz[:, :, 1, :]) & ((xyz[:, :, 0, :] == 0) | (xyz[:, :, 0, :] == n - 1))).any(-1)   # [E, 2]
    assert on_face.all(), (n, int((~on_face).sum()))
    assert (uses <= 2).all()


def test_pattern_coverage():
    """What the fields must contain so that the GPU tests cannot go soft."""
    f = SR.corner_values(FIELDS["noise-18"], LEVEL)
    cell_patterns = np.bincount(((f > 0) * (1 << np.arange(8))).sum(1), minlength=256)
    print("noise-18: rarest cell pattern occurs", int(cell_patterns.min()), "times")
    assert (cell_patterns > 0).all(), np.nonzero(cell_patterns == 0)[0]
    for n in SR.ROUGH_SIZES:
        sig = FIELDS[f"noise-{n}"]
        f = SR.corner_values(sig, LEVEL)
        for t in range(6):
            tet_patterns = np.bincount(((f[:, SR.TET[t]] > 0) * (1 << np.arange(4))).sum(1), minlength=16)
            assert (tet_patterns > 0).all(), (n, t)
        assert SR.cell_face_counts(sig, LEVEL).max() == 12, n
    for n in (2, 3):
        for c in range(8):
            cnt = SR.cell_face_counts(FIELDS[f"one_corner{c}-{n}"], LEVEL)
            assert int(cnt.sum()) == (6 if c in (0, 7) else 2), (n, c)
            assert int((cnt > 0).sum()) == 1                               # all in one cell
        assert SR.cell_face_counts(FIELDS[f"empty-{n}"], LEVEL).sum() == 0
        assert SR.cell_face_counts(FIELDS[f"full-{n}"], LEVEL).sum() == 0
    # the sizes put the scan's edges where the GPU tests need them (2048-element tiles, 8 items per thread)
    assert [(n - 1) ** 3 for n in (2, 3, 14, 17, 18, 82)] == [1, 8, 2197, 4096, 4913, 531441]
    assert 2197 % 8 == 5 and 4096 == 2 * 2048 and -(-531441 // 2048) == 260


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_statistics(seed):
    N = 1 << 18
    w0, w1, w2, g = SR.point_random_numbers(seed, np.arange(N))
    assert w0.dtype == np.float32 and (w0 > 0).all() and (w1 > 0).all() and (w2 > 0).all()
    total = (w0.astype(np.float64) + w1) + w2
    print(f"seed {seed}: |w0 + w1 + w2 - 1| <= {np.abs(total - 1.0).max() / 2.0 ** -24:.2f} x 2^-24")
    # 2 ulp of 1 (2^-23 each): rs carries two roundings of 2^-24 relative, the three quotients half an ulp (<= 2^-25) each
    assert np.abs(total - 1.0).max() <= 2 * 2.0 ** -23
    for k, w in enumerate((w0, w1, w2)):
        w = w.astype(np.float64)
        bar = 5.0 * w.std() / np.sqrt(N)
        print(f"seed {seed} w{k}: mean - 1/3 = {w.mean() - 1 / 3:+.2e}, sd {w.std():.3f}, bar {bar:.2e}")
        assert abs(w.mean() - 1.0 / 3.0) <= bar

    def corr(a, b):
        a, b = a.astype(np.float64), b.astype(np.float64)
        return float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std()))
    lag1, cross = corr(w0[:-1], w0[1:]), corr(w0, g)
    print(f"seed {seed}: lag-1 correlation of w0 {lag1:+.2e}, of w0 with the thickness draw {cross:+.2e}, bar {5 / np.sqrt(N):.2e}")
    assert abs(lag1) <= 5.0 / np.sqrt(N) and abs(cross) <= 5.0 / np.sqrt(N)
    assert np.isfinite(g).all()


@pytest.mark.parametrize("fid", [f for f in FIELDS if not f.startswith(("empty", "full"))])
def test_interpolant_vanishes_on_the_float64_triangles(fid):
    """Reference against itself: the case-table triangles of all_triangles (float64 vertices from float64 corner differences)
    lie in the zero set of the case-free interpolant, to 1e-9 of the field's range."""
    sig = FIELDS[fid]
    tri = SR.all_triangles(sig, LEVEL, corner_dtype=np.float64)
    assert len(tri) == int(SR.cell_face_counts(sig, LEVEL).sum()) > 0
    span = float(sig.max()) - float(sig.min())
    worst = float(np.abs(SR.kuhn_interpolant(sig, LEVEL, tri.reshape(-1, 3))).max())
    print(f"{fid}: worst |interpolant| {worst:.2e} = {worst / span:.2e} of the range")
    assert worst <= 1e-9 * span, (fid, worst, span)


def test_interpolant_bound_is_four_times_the_float32_twin():
    """K of the GPU tests' bound |kuhn_interpolant| <= K 2^-24 n D: the same ratio measured on the float32 restatement's points
    (numbered_faces, the restated weights, the same / n - 0.5 output transform) over every field, level and size the GPU tests
    run, four seeds, 2 F + 3 points each; K = 4 x that maximum.  The maximum is recorded in _surface_ref.K_MEASURED; here it
    is measured again, so the constant cannot drift from the fields."""
    worst = {}
    cases = [(fid, sig, LEVEL) for fid, sig in FIELDS.items()]
    cases += [("noise-9 @ 0", FIELDS["noise-9"] - np.float32(10.0), 0.0), ("noise-9 @ -3", FIELDS["noise-9"] - np.float32(13.0), -3.0)]
    for fid, sig, level in cases:
        faces = SR.numbered_faces(sig, level)
        if len(faces) == 0:
            continue
        seeds = SEEDS if len(faces) < 40000 else (77,)
        worst[fid] = max(float(SR.interpolant_ratio(sig, level, SR.restated_points(sig, level, s, 2 * len(faces) + 3, faces)).max())
                         for s in seeds)
    top = max(worst, key=worst.get)
    print(f"float32 twin: worst ratio {worst[top]:.4f} on {top}; K = {SR.K_INTERPOLANT}")
    print({k: round(v, 3) for k, v in worst.items()})
    assert 0.98 * SR.K_MEASURED <= worst[top] <= SR.K_MEASURED
    assert SR.K_INTERPOLANT == 4.0 * SR.K_MEASURED
