"""The case tables of tests/_teacher_render_cases.py proven on the CPU: every premise the tables state holds for the torch form
(gaussian_gan_decoder_amd/teacher.py: render_teacher_torch, tied to the reference's own outputs by
tests/test_teacher_render_host.py), every constant is what is measured here, and no case needs a ray left out."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import teacher
import _teacher_render_cases as K
import _teacher_render_ref as T


def _np(t):
    return t.detach().cpu().numpy()


def _marched(case):
    """float64 weights of the ordered union's intervals [M, nm], sigma_mid - 1 there and which intervals lie between two samples
    inside the crop, from the torch form's own samples"""
    depths, sigma, _ = K.union(K.reference(case).samples)
    order = np.argsort(depths, 1, kind="stable")
    t, s = np.take_along_axis(depths, order, 1), np.take_along_axis(sigma, order, 1).astype(np.float64)
    inside = s != -1e3
    return T.march(t, s)[0], 0.5 * (s[:, :-1] + s[:, 1:]) - 1.0, inside[:, :-1] & inside[:, 1:]


def test_the_tables_are_the_issue_s_and_none_is_empty():
    assert len(K.TABLE_N) == 2 * 15 and len(K.TABLE_D) == 4 and len(K.TABLE_M) == 10 and len(K.TABLE_C) == 1
    assert len({c.id for c in K.ALL}) == len(K.ALL) == 45
    for f in K.N_FIELDS:
        assert sorted((c.Nc, c.Ni) for c in K.TABLE_N if c.field == f) == sorted(K.N_COUNTS)
    assert sorted(set(K.N_COUNTS.values())) == [3, 4, 6, 63, 64, 65, 67, 126, 127]
    for nm, n in ((63, 4), (64, 2), (65, 2), (126, 2), (127, 1)):
        assert sum(1 for v in K.N_COUNTS.values() if v == nm) == n
    assert sorted({(c.kind, c.Nc, c.Ni) for c in K.TABLE_D}) == [("empty", 33, 33), ("empty", 48, 48), ("opaque", 33, 33),
                                                                 ("opaque", 48, 48)]
    assert sorted({c.M for c in K.TABLE_M if (c.Nc, c.Ni) == (8, 5)}) == [1023, 1024, 1025, 2049, 4099]
    assert {c.M for c in K.TABLE_M if (c.Nc, c.Ni) == (48, 48)} == {1025}
    assert {c.placement for c in K.TABLE_M if c.M >= 1089} == {"front", "tail"}
    assert all(c.placement == "front" for c in K.TABLE_M if c.M <= 1024)
    assert K.TABLE_C[0].M == 1058 and set(K.TOL) == set(K.TABLES) == set(K.MEASURED)
    a, b = (T.case(f) for f in K.N_FIELDS)
    assert (a.crop, a.D, b.crop, b.D) == (0.1, 3, None, 0)


@pytest.mark.parametrize("case", K.TABLE_N + K.TABLE_D, ids=K.ids(K.TABLE_N + K.TABLE_D))
def test_sample_counts_of_tables_n_and_d(case):
    """nm, the shapes the torch form returns, three workgroups of four rays with one live wave in the last"""
    out, b = K.reference(case), K.build(case)
    s = out.samples
    assert case.nm == case.Nc + case.Ni - 1 and (case.table != "N" or case.nm == K.N_COUNTS[(case.Nc, case.Ni)])
    assert s.depths_coarse.shape == (9, case.Nc) and s.depths_fine.shape == (9, case.Ni) and out.features.shape == (9, 32)
    assert case.M == 9 and (case.M + 3) // 4 == 3 and case.M % 4 == 1
    assert np.array_equal(_np(b.origins), b.c.origins[:9]) and np.array_equal(_np(b.dirs), b.c.dirs[:9])
    assert bool((out.weights > 0).all())


@pytest.mark.parametrize("case", K.TABLE_D, ids=K.ids(K.TABLE_D))
def test_density_extremes(case):
    out = K.reference(case)
    w, z, live = _marched(case)
    assert case.nm > 64 and live.any(axis=1).all()
    top = float(out.weights.max())
    print(f"\n  {case.id}: largest weight sum {top:.6g}, weight left to set B {w[:, 64:].sum(1).max():.3e}, sigma_mid - 1 in "
          f"{z[live].min():.2f} .. {z[live].max():.2f}")
    if case.kind == "opaque":
        assert top >= K.OPAQUE_AT_LEAST
        assert (w[:, 64:].sum(1) <= 1e-10).all(), "the transmittance reaches the floor inside set A"
        assert (w[:, :64].sum(1) >= 0.999).all()
        assert (z[live] > 20.0).all(), "softplus takes z > 20 at every interval between two samples inside the crop"
    else:
        assert 0.0 < top <= K.EMPTY_AT_MOST
        assert w.max() <= 1e-5 and (w[live] > 0).all()
        # tiny, yet the float64 restatement stays the yardstick: its 1 - exp(-x) errs by 2^-53 per interval, 1e-8 of a ray's sum
        assert case.nm * 2.0 ** -53 <= 1e-8 * w.sum(1).min()


@pytest.mark.parametrize("case", K.TABLE_M, ids=K.ids(K.TABLE_M))
def test_ray_counts_misses_and_extrema(case):
    out, b = K.reference(case), K.build(case)
    s = out.samples
    M = case.M
    assert set(case.miss) == {r for r in (0, 1023, 1024, M - 1) if r < M} and len(set(case.miss)) == len(case.miss)
    miss = np.zeros(M, bool)
    miss[list(case.miss)] = True
    every = np.concatenate([_np(s.depths_coarse), _np(s.depths_fine)], 1)
    top = every.max()
    # the misses: every sample cropped, weight exactly 0, the background, depth = the call's largest sample depth
    # (some of the fixture's own rays have no two adjacent samples inside the crop box either: whatever has none behaves alike)
    outside = (_np(s.sigma_coarse) == -1e3).all(1) & (_np(s.sigma_fine) == -1e3).all(1)
    zero = _np(out.weights) == 0
    assert outside[miss].all() and zero[outside].all() and int((~zero).sum()) > M // 2
    assert b.white_back and (_np(out.features)[zero] == 1.0).all()
    assert (_np(out.depth)[zero] == top).all() and (_np(out.depth)[~zero] < top).all()
    # the strict extrema, each on one chosen ray
    per_ray_hi, per_ray_lo = every.max(1), every.min(1)
    assert int(per_ray_hi.argmax()) == case.r_hi and (np.delete(per_ray_hi, case.r_hi) < top).all()
    assert int(per_ray_lo.argmin()) == case.r_lo and (np.delete(per_ray_lo, case.r_lo) > every.min()).all()
    assert float(b.u_coarse[case.r_hi, -1]) == K.BELOW_ONE and float(b.u_coarse[case.r_lo, 0]) == 0.0
    assert float(np.delete(_np(b.u_coarse[:, -1]), case.r_hi).max()) <= 0.9
    assert float(np.delete(_np(b.u_coarse[:, 0]), case.r_lo).min()) >= 0.1 and float(b.u_coarse.max()) < 1.0
    if case.placement == "front":
        assert case.r_lo < 1024 and case.r_hi < 1024 and case.r_lo not in case.miss and case.r_hi not in case.miss
    elif case.placement == "tail":
        assert case.r_lo >= 1024 and case.r_hi >= 1024 and K.clamp_wave(case.r_lo) != K.clamp_wave(case.r_hi)
        assert case.r_lo not in case.miss and case.r_hi not in case.miss
    else:
        assert M == 1025 and case.r_lo == case.r_hi == 1024
    # from M = 2049 the second trip of the clamp's stride loop has data in every one of its sixteen waves
    assert M < 2049 or len({K.clamp_wave(r) for r in range(1024, M)}) == 16


def test_the_public_path_case():
    case = K.TABLE_C[0]
    b, out = K.build(case), K.reference(case)
    cams, intr = K.cameras()
    assert cams.shape == (2, 4, 4) and float(intr[:, 0, 1].abs().min()) > 0            # two cameras, both skewed
    assert b.origins.shape == (1058, 3) and b.weights.activation == "sigmoid"
    assert bool((out.weights > 0).all()) and out.samples.depths_fine.shape == (1058, 48)
    o5, d5 = teacher.camera_rays(cams, intr, 5)                                        # the form the fixture ties to the reference
    assert np.array_equal(_np(o5), T.FIX["rays_origins"].reshape(-1, 3)) and np.array_equal(_np(d5), T.FIX["rays_dirs"].reshape(-1, 3))
    a = teacher.render_teacher(b.planes_cl, b.weights, b.origins, b.dirs, generator=torch.Generator().manual_seed(case.seed), **b.kwargs)
    assert torch.equal(a.features, out.features) and torch.equal(a.depth, out.depth)   # draw() is render_teacher's own draw


@pytest.mark.parametrize("case", K.ALL, ids=K.ids(K.ALL))
def test_no_fine_sample_at_the_crop_limit(case):
    """the GPU file's stage checks leave no ray out: judged on the torch form on the CPU"""
    assert case.seed == K.SEED_BASE[case.table] + K.TABLES[case.table].index(case) + K.SEED_MOVED.get(case.id, 0)
    near = K.near_crop(case, K.reference(case).samples.coords_fine)
    assert not near.any(), f"rays {np.nonzero(near)[0].tolist()}: move the seed up by one"


@pytest.mark.parametrize("table", list(K.TABLES))
def test_constants_are_what_is_measured_here(table):
    """neither tighter nor wider: each constant is the table's worst deviation, rounded up in its third digit at most"""
    cases = K.TABLES[table]
    assert cases, "an empty table would measure nothing"
    devs = [K.deviations(c) for c in cases]
    for k in K.STAGES:
        measured, recorded = max(d[k] for d in devs), getattr(K.MEASURED[table], k)
        at = cases[int(np.argmax([d[k] for d in devs]))].id
        print(f"\n  table {table} {k}: measured {measured:.4e} (at {at}), recorded {recorded:.4e}, tolerance {2 * recorded:.4e}")
        assert measured > 0 and measured <= recorded <= 1.01 * measured, k
        assert getattr(K.TOL[table], k) == 2.0 * recorded


def test_the_fine_depths_need_their_own_constant():
    """the bins are wider at Nc = 8: the CPU form alone stands further from float64 there than T.TOL_IMPORTANCE allows"""
    assert K.MEASURED["M"].fine > T.TOL_IMPORTANCE
    for table in ("N", "D", "M", "C"):
        for k in ("features", "weights", "depth"):
            assert getattr(K.MEASURED[table], k) <= getattr(T.TOL_COMPOSITE, k), (table, k)
