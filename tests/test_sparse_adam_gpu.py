"""Sparse Adam on the device (csrc/ggd_adam.hip): bits against the numpy restatement of tests/_sparse_adam_ref.py.

Every comparison is int32-view equality: parameters and both moments of visible rows against the restatement, rows that are
not visible against the inputs.  Through the C entry every array of a case lives in ONE device buffer, each array between
guard words, and the whole buffer is compared, so a store outside an array shows as well.
Row counts 1, 63 / 64 / 65 (a wave), 257 (a workgroup and one row) and 4099 (several workgroups; 3 * 4099, 4099 and 45 * 4099
are no multiples of four floats: a scalar tail); widths 3 and 1 put several rows into one 16-byte chunk.
"""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from _sparse_adam_ref import B1, B2, EPS, LRS, VISIBILITY, adam32, as_radii, draw_grad, draw_group, visibility, widths

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 63, 64, 65, 257, 4099)
GUARD = 4                                                 # floats of guard in front of and behind every array
SENTINEL = np.float32(-12345.678)
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
ATTRS = dict(zip(NAMES, ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")))


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def context():
    from gaussian_gan_decoder_amd import _capi
    cx, stream = _capi.context_and_stream(torch.device(DEV))
    return _capi, cx, C.c_void_p(stream)


class Packed:
    """Arrays laid into one float32 buffer: array k starts `offsets[k]` floats (0..3) behind a 16-byte boundary, with GUARD
    sentinel floats on either side."""

    def __init__(self, arrays, offsets):
        self.at, cursor = [], 0
        for a, off in zip(arrays, offsets):
            start = (cursor + GUARD + 3) // 4 * 4 + off
            self.at.append((start, a.size))
            cursor = start + a.size + GUARD
        self.host = np.full(cursor + 4, SENTINEL, np.float32)
        self.fill(self.host, arrays)

    def fill(self, buf, arrays):
        for (start, n), a in zip(self.at, arrays):
            buf[start:start + n] = a.reshape(-1)

    def upload(self):
        self.dev = torch.from_numpy(self.host).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        return self.dev

    def ptr(self, k):
        return self.dev.data_ptr() + 4 * self.at[k][0]


def run_groups(N, groups, vis, offsets=None, radii=None):
    """groups: [(p, g, m, v, lr, eps)] float32 [N, w] each.  Runs ggd_adam_sparse once and compares the WHOLE buffer with the
    restatement laid out the same way; vis: bool [N]; radii: the int32 form of the same rows, or None for the uint8 form."""
    _capi, cx, st = context()
    arrays = [a for grp in groups for a in grp[:4]]
    offsets = offsets or [0] * len(arrays)
    pk = Packed(arrays, offsets)
    pk.upload()
    table = (_capi.AdamGroup * len(groups))()
    expect = pk.host.copy()
    done = []
    for k, (p, g, m, v, lr, eps) in enumerate(groups):
        slot = table[k]
        slot.param, slot.grad, slot.exp_avg, slot.exp_avg_sq = (pk.ptr(4 * k + j) for j in range(4))
        slot.width, slot.lr, slot.eps = p.size // N, lr, eps
        p1, m1, v1 = adam32(p, g, m, v, vis, lr, eps)
        done += [p1, g, m1, v1]
    pk.fill(expect, done)
    vis_dev = torch.from_numpy(radii if radii is not None else vis.astype(np.uint8)).to(DEV)
    vp = C.c_void_p(vis_dev.data_ptr())
    with torch.cuda.device(DEV):
        rc = cx.lib.ggd_adam_sparse(cx.handle, st, N, len(groups), table, None if radii is not None else vp,
                                    vp if radii is not None else None, B1, B2)
    assert rc == 0, cx.lib.ggd_last_error(cx.handle)
    got = pk.dev.cpu().numpy()
    bad = np.nonzero(bits(got) != bits(expect))[0]
    return bad, got, expect, pk


def six_groups(rng, N, M):
    return [draw_group(rng, N, (w,), lr) + (lr, EPS) for w, lr in zip(widths(M), (1.6e-4, 2.5e-3, 0.0, 0.05, 2.5e-3, 1.6e-4))]


@pytest.mark.parametrize("M", [1, 4, 16])
def test_bit_exact_through_the_c_entry(M):
    cases = 0
    for N in SIZES:
        rng = np.random.default_rng(1000 * M + N)
        groups = six_groups(rng, N, M)
        assert (groups[2][0].shape[1] == 0) == (M == 1)
        for kind in VISIBILITY:
            vis = visibility(kind, N, rng)
            for radii in (None, as_radii(vis, rng)):
                bad, got, expect, _ = run_groups(N, groups, vis, radii=radii)
                assert bad.size == 0, (M, N, kind, radii is not None, bad[:8], got[bad[:8]], expect[bad[:8]])
                cases += 1
    assert cases == len(SIZES) * len(VISIBILITY) * 2


def test_every_learning_rate_and_all_sixteen_byte_phases():
    """Each lr of the input set on each width, and every width-3 / width-1 row phase inside a chunk: N = 4099 rows of width 3
    start at every offset 0..3 of a chunk."""
    rng = np.random.default_rng(7)
    N = 4099
    vis = visibility("random30", N, rng)
    for lr in LRS:
        groups = [draw_group(rng, N, (w,), lr) + (lr, EPS) for w in (1, 3, 4, 45)]
        bad, got, expect, _ = run_groups(N, groups, vis)
        assert bad.size == 0, (lr, bad[:8], got[bad[:8]], expect[bad[:8]])


def test_nothing_leaks_from_invisible_rows():
    for N in (65, 4099):
        rng = np.random.default_rng(N)
        for kind in ("every_other", "random30", "last"):
            vis = visibility(kind, N, rng)
            groups = six_groups(rng, N, 16)
            for p, g, m, v, _, _ in groups:
                hide = ~vis
                g[hide] = np.where(rng.random(g[hide].shape) < 0.5, np.nan, np.inf).astype(np.float32)
                m[hide] = np.where(rng.random(m[hide].shape) < 0.5, np.nan, -np.inf).astype(np.float32)
                v[hide] = np.where(rng.random(v[hide].shape) < 0.5, np.nan, np.inf).astype(np.float32)
            bad, got, expect, pk = run_groups(N, groups, vis, radii=as_radii(vis, rng) if kind == "random30" else None)
            assert bad.size == 0, (N, kind, bad[:8])
            for k, (p, g, m, v, _, _) in enumerate(groups):     # and, spelled out: visible rows finite, the others as they were
                for j, a in ((0, p), (2, m), (3, v)):
                    start, n = pk.at[4 * k + j]
                    out = got[start:start + n].reshape(a.shape)
                    assert np.isfinite(out[vis]).all()
                    assert np.array_equal(bits(out[~vis]), bits(a[~vis]))


@pytest.mark.parametrize("phase", [1, 2, 3, "mixed"])
def test_base_pointers_off_a_sixteen_byte_boundary(phase):
    """Slices of a larger buffer that start 4, 8 and 12 bytes behind a 16-byte boundary (all four arrays of a group alike: the
    chunk form with a scalar head and tail), and a group whose four arrays start at four different phases (run float by
    float).  The guard words around every slice are part of the comparison."""
    for N in (1, 2, 65, 4099):
        rng = np.random.default_rng(10 * N + (phase if phase != "mixed" else 9))
        groups = six_groups(rng, N, 4)
        offsets = [phase] * 24 if phase != "mixed" else [(k + k // 4) % 4 for k in range(24)]
        for kind in ("all", "random30"):
            vis = visibility(kind, N, rng)
            bad, got, expect, pk = run_groups(N, groups, vis, offsets=offsets)
            assert all((start % 4) == off for (start, _), off in zip(pk.at, offsets))
            assert bad.size == 0, (phase, N, kind, bad[:8], got[bad[:8]], expect[bad[:8]])
            for start, n in pk.at:                        # (the guards, spelled out)
                assert (got[start - GUARD:start] == SENTINEL).all() and (got[start + n:start + n + GUARD] == SENTINEL).all()


def test_c_entry_refuses_bad_arguments():
    _capi, cx, st = context()
    lib, h = cx.lib, cx.handle
    N = 100
    buf = torch.full((4 * N * 4,), float(SENTINEL), device=DEV)
    visb = torch.ones((N,), dtype=torch.uint8, device=DEV)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def table(n=1, width=4, skip=None, null=(), grad=True, misalign=None):
        t = (_capi.AdamGroup * max(n, 1))()
        for k in range(max(n, 1)):
            for j, f in enumerate(("param", "grad", "exp_avg", "exp_avg_sq")):
                setattr(t[k], f, None if f in null or (f == "grad" and not grad) else buf.data_ptr() + 16 * N * j + (2 if f == misalign else 0))
            t[k].width, t[k].lr, t[k].eps = (0 if skip == "width" else width), 0.05, EPS
        return t

    second_null = table(2)
    second_null[1].exp_avg = None
    call = lambda n_rows=N, n=1, tab=None, visible=vp(visb), radii=None, ctx=h: lib.ggd_adam_sparse(
        ctx, st, n_rows, n, tab if tab is not None else table(n), visible, radii, B1, B2)
    with torch.cuda.device(DEV):
        bad = {"NULL ctx": call(ctx=None), "N < 0": call(n_rows=-1), "N > 2^26": call(n_rows=(1 << 26) + 1),
               "n_groups 0": call(n=0), "n_groups 9": call(n=9, tab=table(9)), "n_groups -1": call(n=-1),
               "both": call(radii=vp(visb)), "neither": call(visible=None), "NULL table": lib.ggd_adam_sparse(h, st, N, 1, None, vp(visb), None, B1, B2),
               "NULL param": call(tab=table(null=("param",))), "NULL exp_avg": call(tab=table(null=("exp_avg",))),
               "NULL exp_avg_sq": call(tab=table(null=("exp_avg_sq",))), "width < 0": call(tab=table(width=-1)),
               "N * width = 2^31": call(n_rows=1 << 26, tab=table(width=32)),
               "second group NULL": call(n=2, tab=second_null), "misaligned": call(tab=table(misalign="grad"))}
        ok = {"N == 0": call(n_rows=0), "all skipped by grad": call(tab=table(grad=False)),
              "all skipped by width": call(tab=table(skip="width")), "two skipped": call(n=2, tab=table(2, grad=False))}
    torch.cuda.synchronize()
    assert {k: v for k, v in bad.items() if v == 0} == {}
    assert {k: v for k, v in bad.items() if k != "NULL ctx" and v != -1} == {}
    assert {k: v for k, v in ok.items() if v != 0} == {}
    assert call(visible=None) != 0 and b"visible" in lib.ggd_last_error(h)
    assert bool((buf == float(SENTINEL)).all()) and bool((visb == 1).all())      # nothing was launched


def test_optimizer_three_steps_with_a_group_without_gradient():
    from gaussian_gan_decoder_amd.sparse_adam import SparseGaussianAdam
    rng = np.random.default_rng(5)
    N = 257
    shapes = {"a": (3,), "b": (15, 3), "c": (1,), "idle": (4,)}
    lrs = {"a": 1.6e-4, "b": 2.5e-3, "c": 0.05, "idle": 0.05}
    host = {n: rng.standard_normal((N,) + s).astype(np.float32) for n, s in shapes.items()}
    params = {n: torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for n, a in host.items()}
    opt = SparseGaussianAdam([{"params": [params[n]], "lr": lrs[n], "name": n} for n in shapes], lr=0.0, eps=EPS)
    assert len(opt.state) == 0
    ref = {n: (host[n], np.zeros_like(host[n]), np.zeros_like(host[n])) for n in ("a", "b", "c")}
    forms = (lambda v: torch.from_numpy(v), lambda v: torch.from_numpy(v.astype(np.uint8)), lambda v: torch.from_numpy(as_radii(v, rng)))
    for step, kind in enumerate(("random30", "every_other", "random30")):
        vis = visibility(kind, N, rng)
        if step == 1:
            opt.param_groups[0]["lr"] = lrs["a"] = 3.0e-4    # the rate is read from the group at every step
        for n in ("a", "b", "c"):
            g = draw_grad(rng, host[n].shape)
            params[n].grad = torch.from_numpy(g).to(DEV)
            if n == "b" and step == 2:                    # a gradient with other strides is made contiguous
                params[n].grad = params[n].grad.transpose(1, 2).contiguous().transpose(1, 2)
                assert not params[n].grad.is_contiguous()
            ref[n] = adam32(ref[n][0], g, ref[n][1], ref[n][2], vis, lrs[n])
        opt.step(forms[step](vis).to(DEV), N)
        for n in ("a", "b", "c"):
            st = opt.state[params[n]]
            assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 0.0 and st["step"].dtype == torch.float32
            assert st["exp_avg"].shape == params[n].shape
            for got, want in zip((params[n].detach(), st["exp_avg"], st["exp_avg_sq"]), ref[n]):
                assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (step, n)
    assert params["idle"] not in opt.state
    assert np.array_equal(bits(params["idle"].detach().cpu().numpy()), bits(host["idle"]))
    # checks that run before anything is launched
    before = bits(params["a"].detach().cpu().numpy()).copy()
    ones = torch.ones(N, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError):
        opt.step(ones[:-1], N)
    with pytest.raises(ValueError):
        opt.step(ones.float(), N)
    with pytest.raises(ValueError):
        opt.step(ones, N - 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step(ones.cpu(), N)
    wide = torch.nn.Parameter(torch.zeros(N, 3, device=DEV, dtype=torch.float64))
    wide.grad = torch.ones_like(wide)
    with pytest.raises(ValueError, match="float32"):
        SparseGaussianAdam([{"params": [wide]}], lr=0.1, eps=EPS).step(ones, N)
    ragged = torch.nn.Parameter(torch.zeros(N + 1, device=DEV))
    ragged.grad = torch.ones_like(ragged)
    with pytest.raises(ValueError, match="multiple"):
        SparseGaussianAdam([{"params": [ragged]}], lr=0.1, eps=EPS).step(ones, N)
    strided = torch.nn.Parameter(torch.zeros(3, N, device=DEV).t())
    strided.grad = torch.ones(N, 3, device=DEV)
    with pytest.raises(ValueError, match="contiguous"):
        SparseGaussianAdam([{"params": [strided]}], lr=0.1, eps=EPS).step(ones, N)
    assert not wide.any() and not ragged.any() and not strided.any()
    two =SparseGaussianAdam([{"params": [torch.nn.Parameter(torch.zeros(N, 3, device=DEV)), torch.nn.Parameter(torch.zeros(N, 1, device=DEV))]}],
                             lr=0.1, eps=EPS)
    with pytest.raises(ValueError, match="one tensor per group"):
        two.step(ones, N)
    torch.cuda.synchronize()
    assert np.array_equal(bits(params["a"].detach().cpu().numpy()), before)


def training_args(**over):
    a = dict(percent_dense=0.01, position_lr_init=0.002, position_lr_final=0.0002, position_lr_delay_mult=0.01,
             position_lr_max_steps=30_000, feature_lr=0.02, opacity_lr=0.1, scaling_lr=0.01, rotation_lr=0.001)
    a.update(over)
    return SimpleNamespace(**a)


def snapshot(pc):
    """name -> (parameter, exp_avg, exp_avg_sq) on the host; zeros for a group without state."""
    out = {}
    for n, attr in ATTRS.items():
        p = getattr(pc, attr)
        st = pc.optimizer.state.get(p) or {}
        mom = [st[k].cpu().numpy().copy() if k in st else np.zeros(tuple(p.shape), np.float32) for k in ("exp_avg", "exp_avg_sq")]
        out[n] = (p.detach().cpu().numpy().copy(), mom[0], mom[1])
    return out


def fitted_iteration(pc, sc, target, pipe, it, expect_both=True):
    """One iteration of the fitting loop with the sparse step, compared against the restatement; returns the visible rows."""
    from gaussian_gan_decoder_amd.gaussian_renderer import render
    pc.update_learning_rate(it)
    out = render(sc.cam, pc, pipe, sc.bg)
    loss = (out["render"] - target).abs().mean()
    loss.backward()
    with torch.no_grad():
        pc.update_densification_stats(out["viewspace_points"], out["radii"])
        P = out["radii"].shape[0]
        before = snapshot(pc)
        grads = {n: getattr(pc, attr).grad.cpu().numpy().copy() for n, attr in ATTRS.items()}
        vis = (out["radii"] > 0).cpu().numpy()
        if expect_both:
            assert vis.any() and not vis.all(), int(vis.sum())
        pc.optimizer.step(out["radii"], P)
        pc.optimizer.zero_grad(set_to_none=True)
        after = snapshot(pc)
    lrs = {g["name"]: g["lr"] for g in pc.optimizer.param_groups}
    for n in NAMES:
        want = adam32(before[n][0], grads[n], before[n][1], before[n][2], vis, lrs[n])
        for k, what in enumerate(("parameter", "exp_avg", "exp_avg_sq")):
            assert after[n][k].shape == before[n][k].shape
            assert np.array_equal(bits(after[n][k][~vis]), bits(before[n][k][~vis])), (it, n, what, "a row the frame did not see moved")
            assert np.array_equal(bits(after[n][k]), bits(want[k])), (it, n, what)
        assert "step" in pc.optimizer.state[getattr(pc, ATTRS[n])]
    assert any(not np.array_equal(after[n][0], before[n][0]) for n in NAMES)
    return vis


def test_fitting_loop_end_to_end():
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    from gaussian_gan_decoder_amd.gaussian_renderer import render
    from gaussian_gan_decoder_amd.sparse_adam import SparseGaussianAdam
    from gaussian_gan_decoder_amd.synthetic import make_scene
    pipe = SimpleNamespace(debug=False, compute_cov3D_python=False, convert_SHs_python=False)
    sc = make_scene(2000, 64, "cube", seed=3, log_scale_mean=-4.0).to(DEV)
    with torch.no_grad():
        target = render(sc.cam, sc.gaussian_model(), pipe, sc.bg)["render"].clone()
    # the scene's own small scales (three sigma of about 0.05) instead of the nearest-neighbour seeds, which would reach the
    # 12-degree frustum (half width 0.28 at the cube's centre) from anywhere in the cube: rows outside it have radii == 0
    seed = make_scene(256, 64, "cube", seed=11, log_scale_mean=-4.0)
    gen = torch.Generator().manual_seed(0)
    pc = GaussianModel(1)
    pc.create_from_pos_col(seed.xyz.to(DEV), torch.rand((256, 3), generator=gen).to(DEV), scaling=seed.log_scales.to(DEV))
    pc.oneupSHdegree()
    args = training_args(optimizer_type="sparse_adam")
    pc.training_setup(args)
    assert type(pc.optimizer) is SparseGaussianAdam and len(pc.optimizer.state) == 0
    for it in (1, 2):
        fitted_iteration(pc, sc, target, pipe, it)
    pc.reset_opacity()
    st = pc.optimizer.state[pc._opacity]
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and st["exp_avg"].shape == pc._opacity.shape
    assert pc.get_opacity.max().item() <= 0.01 * (1 + 1e-5)
    fitted_iteration(pc, sc, target, pipe, 3)
    P0 = pc.get_xyz.shape[0]
    pc.densify_and_prune(1e-12, 0.005, 1.0, None, noise=torch.randn((2, P0, 3), device=DEV, generator=torch.Generator(DEV).manual_seed(4)))
    P1 = pc.get_xyz.shape[0]
    assert P1 != P0, (P0, P1)
    for attr in ATTRS.values():
        p = getattr(pc, attr)
        st = pc.optimizer.state[p]
        assert p.shape[0] == P1 and st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and "step" in st
    fitted_iteration(pc, sc, target, pipe, 4)
    fresh = GaussianModel(1)
    fresh.restore(copy.deepcopy(pc.capture()), args)
    assert type(fresh.optimizer) is type(pc.optimizer) is SparseGaussianAdam and fresh._xyz is not pc._xyz
    for attr in ATTRS.values():
        a, b = fresh.optimizer.state[getattr(fresh, attr)], pc.optimizer.state[getattr(pc, attr)]
        assert set(a) == set(b) == {"step", "exp_avg", "exp_avg_sq"} and float(a["step"]) == float(b["step"])
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    assert [g["lr"] for g in fresh.optimizer.param_groups][1:] == [g["lr"] for g in pc.optimizer.param_groups][1:]
    fitted_iteration(fresh, sc, target, pipe, 5)          # and the restored optimizer steps
    mask = torch.zeros(P1, dtype=torch.bool, device=DEV)
    mask[::3] = True
    pc.prune_points(mask)
    assert pc.get_xyz.shape[0] == P1 - int(mask.sum()) == pc.optimizer.state[pc._rotation]["exp_avg"].shape[0]
    fitted_iteration(pc, sc, target, pipe, 5, expect_both=False)


def test_default_optimizer_on_the_device_is_torch_adam():
    from gaussian_gan_decoder_amd.gaussian_model import GaussianModel
    pc = GaussianModel(0)
    pc.create_from_pos_col(torch.rand((64, 3), generator=torch.Generator().manual_seed(0)).to(DEV))
    args = training_args()
    assert not hasattr(args, "optimizer_type")
    pc.training_setup(args)
    assert type(pc.optimizer) is torch.optim.Adam
    assert [g["name"] for g in pc.optimizer.param_groups] == list(NAMES)
    pc._xyz.grad = torch.ones_like(pc._xyz)
    before = pc._xyz.detach().clone()
    pc.optimizer.step()                                   # the stock signature, the stock bias-corrected first step: -lr * sign(g)
    assert torch.allclose(pc._xyz.detach(), before - 0.002, rtol=0, atol=1e-6)
    assert float(pc.optimizer.state[pc._xyz]["step"]) == 1.0
