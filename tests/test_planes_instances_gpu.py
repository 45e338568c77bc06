"""Every kernel instance and edge of csrc/ggd_triplane.hip (ggd_planes_gather / ggd_planes_scatter) against the float64
restatement of tests/_planes_ref.py, element by element:  |gpu - ref64| <= 1e-7 + KAPPA * 2^-24 * budget, no array-scale
term, elements of zero budget exactly 0.  The case table, the budgets and where KAPPA comes from: tests/_planes_ref.py;
tests/test_planes_ref_host.py checks on the host that every case hits the edge it is named for.

Groups: A every instance of the plain forms (plane_kernel<C, G3, BACKWARD>, and gather4_kernel<C, G3> for C >= 16); B wave / workgroup edges with sentinel rows (direct calls); C the sorted-run
backward against the plain one on both sides of SR_MIN_POINTS, modulation in LDS and in memory; D kept-item counts on and
next to the chunk and stream edges; E 65 launched / 64 live sort tiles; F run lengths; G accumulate; H refusals."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import _capi
from gaussian_gan_decoder_amd.decoder import planes_channels_last, planes_gather
import _planes_ref as R

DEV = torch.device("cuda:0")
AXES = {"eg3d": 0, "panohead": 1}
_ids = dict(ids=lambda c: c.name)


def _ref(c):
    """float64 (feat, grad, fbud, gbud) of a case, evaluated on the device"""
    return R.reference_of(c, "cuda:0")


def _inputs(c):
    b = R.build(c)
    return SimpleNamespace(planes=b.planes.to(DEV), pos=b.pos.to(DEV), gout=b.gout.to(DEV),
                           mod=None if b.mod is None else b.mod.to(DEV))


def _autograd(c):
    """features and plane gradient through planes_channels_last / planes_gather and autograd"""
    b = _inputs(c)
    planes = b.planes.requires_grad_(True)
    out = planes_gather(planes_channels_last(planes, c.D or None), b.pos, c.box_warp, c.axes, c.D or None, mod=b.mod)
    assert out.shape == (c.N, c.C)
    out.backward(b.gout)
    return out.detach(), planes.grad


def _check_autograd(c):
    out, grad = _autograd(c)
    feat, gref, fbud, gbud = _ref(c)
    R.assert_within(out, feat, fbud, c.name + " features")
    R.assert_within(grad, gref, gbud, c.name + " plane gradient")


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _cx():
    return _capi.context_for(DEV), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _gather(a):
    cx, stream = _cx()
    with torch.cuda.device(DEV):
        return cx.lib.ggd_planes_gather(cx.handle, stream, _vp(a.grids), a.C, a.D, a.H, a.W, a.axes, _vp(a.mod), _vp(a.pos), a.N,
                                        a.box_warp, _vp(a.out))


def _scatter(a):
    cx, stream = _cx()
    with torch.cuda.device(DEV):
        return cx.lib.ggd_planes_scatter(cx.handle, stream, a.C, a.D, a.H, a.W, a.axes, _vp(a.mod), _vp(a.pos), a.N, a.box_warp,
                                         _vp(a.dout), _vp(a.dgrids), a.accumulate)


def _direct_args(c, b):
    """the arguments of a direct call for a case; out / dgrids are the caller's to fill in"""
    return SimpleNamespace(grids=planes_channels_last(b.planes, c.D or None), C=c.C, D=c.D, H=c.H, W=c.W, axes=AXES[c.axes],
                           mod=b.mod, pos=b.pos, N=c.N, box_warp=c.box_warp, out=None, dout=b.gout, dgrids=None, accumulate=0)


def _bits(t):
    return t.view(torch.int32)


# ---- A: every instance of the plain forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.group("A"), **_ids)
def test_every_plain_instance_matches_float64(native_lib, c):
    """C in {1 .. 64} x {planes, eg3d grid D = 3, panohead grid D = 2} x {plain, modulated}, 12 x 20 texels so that an H / W swap
    shows, N = 2051 (the plain scatter-add), box_warp 0.7 / 4.0: forward and backward."""
    _check_autograd(c)


# ---- B: wave and workgroup edges -----------------------------------------------------------------------------------------------
def _pool(c):
    """a group-B case with the B_SENTINEL_ROWS rows of its pool that follow row N"""
    full = c._replace(N=c.N + R.B_SENTINEL_ROWS)
    b = R.build(full)
    return SimpleNamespace(planes=b.planes.to(DEV), pos=b.pos.to(DEV), gout=b.gout.to(DEV),
                           mod=None if b.mod is None else b.mod.to(DEV))


@pytest.mark.parametrize("c", R.group("Bg"), **_ids)
def test_gather_stops_at_row_n(native_lib, c):
    """N on and next to the points of one wave and of one workgroup: rows < N within budget, the 64 rows behind them (valid
    positions are there to be read) bit-unchanged."""
    cx, _ = _cx()
    b = _pool(c)
    a = _direct_args(c, b)
    a.out = torch.full((c.N + R.B_SENTINEL_ROWS, c.C), float("nan"), device=DEV)
    sentinel = torch.randn(R.B_SENTINEL_ROWS, c.C, device=DEV)
    a.out[c.N:] = sentinel
    cx.check(_gather(a))
    feat, _, fbud, _ = _ref(c)
    assert torch.equal(_bits(a.out[c.N:]), _bits(sentinel))
    R.assert_within(a.out[:c.N], feat, fbud, c.name + " features")


@pytest.mark.parametrize("c", R.group("Bs"), **_ids)
def test_scatter_stops_at_row_n(native_lib, c):
    """The same edges for the scatter: the rows of dout behind row N are NaN (with valid positions next to them), the
    gradient buffer is NaN-filled before the call."""
    cx, _ = _cx()
    b = _pool(c)
    a = _direct_args(c, b)
    a.dout = b.gout.clone()
    a.dout[c.N:] = float("nan")
    a.dgrids = torch.full_like(a.grids, float("nan"))
    cx.check(_scatter(a))
    _, gref, _, gbud = _ref(c)
    R.assert_within(a.dgrids, R.channels_last(gref, c.D), R.channels_last(gbud, c.D), c.name + " gradient")


# ---- C: the sorted-run backward and the plain one, on both sides of the switch ----------------------------------------------------
@pytest.mark.parametrize("c", R.group("C"), **_ids)
def test_both_backward_forms_match_float64_at_the_switch(native_lib, c):
    """N = SR_MIN_POINTS (sorted runs) and SR_MIN_POINTS - 1 (plain scatter-add) over the same leading points: no modulation,
    the table in LDS (D * C <= SR_MOD_LDS) and read from memory (D * C > SR_MOD_LDS, 6 x 6 x D grids)."""
    _check_autograd(c)


# ---- D: kept-item counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.group("D"), **_ids)
def test_kept_item_counts_on_the_chunk_and_stream_edges(native_lib, c):
    """kept items in {0, 1, SR_CHUNK - 1 .. 4 SR_CHUNK + 1, 3 N - 1} for C = 16 (four streams per wave) and C = 64 (one);
    kept = 0: an all-zero gradient (every budget is 0), and accumulate = 1 leaves a prefilled buffer bit-unchanged."""
    _check_autograd(c)
    if c.kept == 0:
        cx, _ = _cx()
        a = _direct_args(c, _inputs(c))
        prefill = torch.randn_like(a.grids)
        a.dgrids, a.accumulate = prefill.clone(), 1
        cx.check(_scatter(a))
        assert torch.equal(_bits(a.dgrids), _bits(prefill))


# ---- E: look-back group rows ------------------------------------------------------------------------------------------------------
def test_sorted_scatter_with_65_launched_and_64_live_sort_tiles(native_lib):
    """The 257 / 256 regression of tests/test_decoder_gpu.py (status words laid out for the launched tile count, look-back
    groups sized from the live one) at the next smaller power of four: 3 N = 264 000 items = 65 tiles, 64 of them live."""
    _check_autograd(R.BY_NAME["E-lookback-65-64"])


# ---- F: run lengths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.group("F"), **_ids)
def test_run_lengths_from_one_to_everything(native_lib, c):
    """one cell holding every point (one run across every stream, wave and workgroup), one position, and 256 x 256 texels
    under uniform points (runs of one or two items)"""
    _check_autograd(c)


# ---- G: accumulate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.ACCUMULATE_CASES, **_ids)
def test_accumulate_adds_and_overwrite_overwrites(native_lib, c):
    """accumulate = 1 onto random values == prefill + gradient within budget + |prefill| * 2^-24 (the sum's own rounding);
    accumulate = 0 overwrites a NaN-filled buffer completely.  Plain and sorted form."""
    cx, _ = _cx()
    a = _direct_args(c, _inputs(c))
    _, gref, _, gbud = _ref(c)
    gref, gbud = R.channels_last(gref, c.D), R.channels_last(gbud, c.D)
    prefill = torch.randn_like(a.grids)
    a.dgrids, a.accumulate = prefill.clone(), 1
    cx.check(_scatter(a))
    R.assert_within(a.dgrids, prefill.double().view(gref.shape) + gref, gbud, c.name + " accumulate = 1",
                    extra=prefill.double().abs() * R.U)
    a.dgrids, a.accumulate = torch.full_like(a.grids, float("nan")), 0
    cx.check(_scatter(a))
    R.assert_within(a.dgrids, gref, gbud, c.name + " accumulate = 0")


# ---- H: refusals -------------------------------------------------------------------------------------------------------------------
_BAD = [("C0", dict(C=0)), ("C3", dict(C=3)), ("C48", dict(C=48)), ("C128", dict(C=128)), ("axes2", dict(axes=2)),
        ("Dneg", dict(D=-1)), ("D0-panohead-axes", dict(D=0, axes=1)), ("box_warp0", dict(box_warp=0.0)),
        ("null-pos", dict(pos=None))]


def _refusal_args():
    g = torch.Generator().manual_seed(7)
    N, Cmax, D, H, W = 100, 128, 2, 12, 20
    return SimpleNamespace(grids=torch.randn(3, D, H, W, Cmax, generator=g).to(DEV), C=32, D=D, H=H, W=W, axes=0, mod=None,
                           pos=(torch.rand(N, 3, generator=g) - 0.5).to(DEV), N=N, box_warp=1.0,
                           out=torch.randn(N, Cmax, generator=g).to(DEV), dout=torch.randn(N, Cmax, generator=g).to(DEV),
                           dgrids=torch.randn(3, D, H, W, Cmax, generator=g).to(DEV), accumulate=0)


def _assert_refused(rc):
    cx, _ = _cx()
    assert rc != 0
    with pytest.raises(_capi.RasterError):
        cx.check(rc)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,bad", _BAD + [("null-out", dict(out=None))], ids=lambda v: v if isinstance(v, str) else "")
def test_gather_refuses_bad_arguments_and_leaves_out_alone(native_lib, name, bad):
    a = _refusal_args()
    before = a.out.clone()
    vars(a).update(bad)
    _assert_refused(_gather(a))
    assert torch.equal(_bits(before), _bits(a.out if a.out is not None else before))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name,bad", _BAD + [("null-dout", dict(dout=None)), ("null-dgrids", dict(dgrids=None))],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_scatter_refuses_bad_arguments_and_leaves_the_gradient_buffer_alone(native_lib, name, bad, accumulate):
    """also with accumulate = 0: a refused call must not have cleared the caller's buffer on the way"""
    a = _refusal_args()
    a.accumulate = accumulate
    buf, before = a.dgrids, a.dgrids.clone()
    vars(a).update(bad)
    _assert_refused(_scatter(a))
    assert torch.equal(_bits(before), _bits(buf))
