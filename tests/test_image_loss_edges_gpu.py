"""The fused image loss (csrc/ggd_imgloss.hip through losses.fused_image_loss and through the C ABI) term by term against the
float64 restatement at tile, window and block edges: the table, the bounds and their derivation are in
tests/_image_loss_cases.py, their soundness in tests/test_image_loss_cases_host.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gaussian_gan_decoder_amd import losses as L
import _image_loss_cases as IC
import _masked_loss_ref as MR

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "masked_losses.npz"))
DEV = torch.device("cuda:0")
ONE_HOT = ("l1", "l2", "ssim", "sobel")


def _kw(wname):
    return dict(zip(("l1_weight", "l2_weight", "ssim_weight", "sobel_weight"), IC.WEIGHTS[wname]))


def _piece(key):
    return IC.equal_piece_max(key[0], key[1]) if key[2] == "equal" else None


def _worse(worst, ratios):
    for n, v in ratios.items():
        worst[n] = max(worst.get(n, 0.0), v)


def _fmt(ratios):
    return ", ".join(f"{n} {v:.3f}" for n, v in ratios.items())


def _run(img, tgt, wname, factor, mask=None):
    """(terms[5], image.grad) as numpy from one wrapper call with `factor` as the upstream gradient of the total."""
    x = img.to(DEV).requires_grad_(True)
    total, terms = L.fused_image_loss(x, tgt.to(DEV), mask=mask, **_kw(wname))
    total.backward(torch.tensor(factor, device=DEV))
    assert float(total.detach()) == float(terms[4])
    return terms.cpu().numpy(), x.grad.cpu().numpy()


@pytest.mark.parametrize("wname", list(IC.WEIGHTS))
def test_each_term_matches_float64(native_lib, wname):
    """Every shape x variant of the table with one weight vector (the four one-hot vectors: each gradient on its own, not under
    the Sobel gradient of the sum), upstream factor -2.5.  Prints the worst error / bound per term, and what the float32
    restatement on this machine's CPU uses of the same bounds."""
    worst, worst_dev = {}, {}
    for key in IC.keys():
        ref = IC._ref(*key, wname)
        terms, grad = _run(*IC.case(*key), wname, -2.5)
        _worse(worst, IC.judge(ref, wname, terms, grad, factor=-2.5, piece_max=_piece(key), what=key))
        _worse(worst_dev, IC.dev_ratios(ref, wname, _piece(key)))
    print(f"\n  weights {wname}: worst kernel error / bound: {_fmt(worst)}\n  weights {wname}: worst float32-restatement "
          f"deviation / bound: {_fmt(worst_dev)}")


@pytest.mark.parametrize("tag", MR.CASES)
def test_masked_terms_one_by_one(native_lib, tag):
    """The masked instances on the cases of tests/golden/masked_losses.npz with each one-hot weight vector against the float64
    restatement, by the rules of the unmasked table with dev32 computed here for that weight vector (the stored *_dev_grad
    belongs to the summed gradient).  The gradient is exactly 0 wherever the upsampled mask is 0, for each weight on its own."""
    img, tgt, mask = (torch.from_numpy(GOLD[f"{tag}_{k}"]) for k in ("image", "target", "mask"))
    zero = np.broadcast_to(GOLD[f"{tag}_upmask"] == 0, img.shape)
    assert zero.any()
    worst, worst_dev = {}, {}
    for wname in ONE_HOT:
        ref = IC.evaluate(img, tgt, IC.WEIGHTS[wname], mask)
        terms, grad = _run(img, tgt, wname, -2.5, mask=mask.to(DEV))
        r = IC.judge(ref, wname, terms, grad, factor=-2.5, what=(tag, wname))
        k = ONE_HOT.index(wname)
        worst[IC.TERM_NAMES[k]], worst[f"grad {wname}"] = r[IC.TERM_NAMES[k]], r["grad"]
        d = IC.dev_ratios(ref, wname)
        worst_dev[IC.TERM_NAMES[k]], worst_dev[f"grad {wname}"] = d[IC.TERM_NAMES[k]], d["grad"]
        assert (grad[zero] == 0.0).all() and (grad[~zero] != 0.0).any(), (tag, wname)
    print(f"\n  masked case {tag}: kernel error / bound: {_fmt(worst)}\n  masked case {tag}: float32-restatement deviation / "
          f"bound: {_fmt(worst_dev)}")


GUARD = 64                 # guard words on each side
SENTINEL = 0x5A5A5A5A      # a finite float (1.5e16) that no result equals


class _Guarded:
    """`n` float32 in the middle of a larger sentinel-filled buffer, starting 4 bytes past a 256-byte boundary."""

    def __init__(self, n, fill=None):
        self.buf = torch.empty(n + 2 * GUARD + 64, dtype=torch.int32, device=DEV).fill_(SENTINEL)
        self.start = next(i for i in range(GUARD, GUARD + 64) if (self.buf.data_ptr() + 4 * i) % 256 == 4)
        self.data = self.buf.view(torch.float32)[self.start:self.start + n]
        if fill is not None:
            self.data.copy_(fill.reshape(-1)) if torch.is_tensor(fill) else self.data.fill_(fill)
        assert self.data.data_ptr() % 256 == 4

    def guards_intact(self):
        n = self.data.numel()
        return bool((self.buf[:self.start] == SENTINEL).all()) and bool((self.buf[self.start + n:] == SENTINEL).all())


def _abi_buffers(H, W, img, tgt):
    """The guarded (image, target, gradient, terms) buffers of one call: inputs copied in, outputs NaN."""
    return (_Guarded(3 * H * W, img.to(DEV)), _Guarded(3 * H * W, tgt.to(DEV)), _Guarded(3 * H * W, float("nan")),
            _Guarded(5, float("nan")))


def _abi_launch(cx, H, W, bufs, wname, tmp, tmp_bytes):
    """Enqueues one ggd_image_loss on the current stream; no host wait."""
    gi, gt, gg, g5 = bufs
    w4 = (C.c_float * 4)(*IC.WEIGHTS[wname])
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    cx.check(cx.lib.ggd_image_loss(cx.handle, stream, W, H, p(gi.data), p(gt.data), w4, p(g5.data), p(gg.data), p(tmp), tmp_bytes))


def _abi_judge(key, wname, img, tgt, bufs):
    gi, gt, gg, g5 = bufs
    H, W, _ = key
    r = IC.judge(IC._ref(*key, wname), wname, g5.data.cpu().numpy(), gg.data.cpu().numpy().reshape(3, H, W), piece_max=_piece(key),
                 what=key)
    assert all(b.guards_intact() for b in bufs), key
    assert torch.equal(gi.data.cpu(), img.reshape(-1)) and torch.equal(gt.data.cpu(), tgt.reshape(-1)), key
    return r


@pytest.mark.parametrize("shape", [(33, 31), (1, 1), (3, 65), (70, 97)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_c_abi_writes_what_it_owns(native_lib, shape):
    """ggd_image_loss on pointers that are only float-aligned (4 bytes past a 256-byte boundary), gradient and terms
    pre-filled with NaN, scratch of exactly ggd_image_loss_tmp_bytes filled with 0xFF bytes (NaN as floats): every gradient
    element and all five terms are written and within the table's bounds, and no guard word around the gradient, the terms,
    the inputs or behind the scratch changes."""
    from gaussian_gan_decoder_amd import _capi
    cx = _capi.context_for(DEV)
    H, W = shape
    nbytes = int(cx.lib.ggd_image_loss_tmp_bytes(W, H))
    assert nbytes >= 64 + 11 * 4 * H * W
    tail = 1024
    tmp = torch.empty(nbytes + tail, dtype=torch.uint8, device=DEV)
    tmp[:nbytes] = 0xFF
    tmp[nbytes:] = 0xA5
    for variant, wname in (("tex", "train"), ("equal", "ssim")):
        key = (H, W, variant)
        img, tgt = IC.case(*key)
        bufs = _abi_buffers(H, W, img, tgt)
        _abi_launch(cx, H, W, bufs, wname, tmp, nbytes)
        torch.cuda.synchronize()
        _abi_judge(key, wname, img, tgt, bufs)
        assert bool((tmp[nbytes:] == 0xA5).all()), key
        tmp[:nbytes] = 0xFF


def test_scratch_is_reused_across_sizes(native_lib):
    """One scratch buffer sized for (70, 97), never cleared by the caller, serves (70, 97), (7, 1) and (32, 33) enqueued back to
    back on one stream with no host wait in between; each call has its own outputs and stays within its own bounds."""
    from gaussian_gan_decoder_amd import _capi
    cx = _capi.context_for(DEV)
    nbytes = int(cx.lib.ggd_image_loss_tmp_bytes(97, 70))
    tmp = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    keys = [(70, 97, "tex"), (7, 1, "tex"), (32, 33, "over")]
    calls = [_abi_buffers(k[0], k[1], *IC.case(*k)) for k in keys]
    torch.cuda.synchronize()
    for k, bufs in zip(keys, calls):                  # three enqueues, nothing else in between
        _abi_launch(cx, k[0], k[1], bufs, "train", tmp, nbytes)
    torch.cuda.synchronize()
    for k, bufs in zip(keys, calls):
        _abi_judge(k, "train", *IC.case(*k), bufs)


def test_wrapper_layouts_and_scales(native_lib):
    """losses.fused_image_loss away from a contiguous float32 leaf and a positive upstream factor: a crop view, a permuted view, a
    float64 image, upstream factors 0 and -1, all-zero weights, and a side stream."""
    key = (33, 31, "tex")
    H, W, _ = key
    img, tgt = IC.case(*key)
    ref = IC._ref(*key, "train")
    tgt_d = tgt.to(DEV)

    # a non-contiguous crop of a leaf: the leaf's gradient is the crop's inside and exactly 0 outside
    big = torch.full((3, 40, 40), 0.5)
    big[:, 2:35, 3:34] = img
    big = big.to(DEV).requires_grad_(True)
    view = big[:, 2:35, 3:34]
    assert not view.is_contiguous()
    total, terms = L.fused_image_loss(view, tgt_d, **_kw("train"))
    total.backward()
    g = big.grad.cpu().numpy()
    IC.judge(ref, "train", terms.cpu().numpy(), g[:, 2:35, 3:34], what="crop")
    outside = np.ones(g.shape, dtype=bool)
    outside[:, 2:35, 3:34] = False
    assert (g[outside] == 0.0).all() and float(total) == float(terms[4])

    # a permuted HWC -> CHW view (image and target)
    hwc = img.permute(1, 2, 0).contiguous().to(DEV).requires_grad_(True)
    chw = hwc.permute(2, 0, 1)
    assert not chw.is_contiguous()
    total, terms = L.fused_image_loss(chw, tgt.permute(1, 2, 0).contiguous().to(DEV).permute(2, 0, 1), **_kw("train"))
    total.backward()
    IC.judge(ref, "train", terms.cpu().numpy(), hwc.grad.permute(2, 0, 1).cpu().numpy(), what="permuted")

    # a float64 image that is not representable in float32: the reference is taken at image.float()
    img64 = img.double() * (1.0 + 2.0 ** -30)
    assert not torch.equal(img64.float().double(), img64)
    ref64 = IC.evaluate(img64.float(), tgt, IC.WEIGHTS["train"])
    x = img64.to(DEV).requires_grad_(True)
    total, terms = L.fused_image_loss(x, tgt_d.double(), **_kw("train"))
    total.backward()
    assert x.grad.dtype == torch.float64 and torch.equal(x.grad.float().double(), x.grad) and terms.dtype == torch.float32
    IC.judge(ref64, "train", terms.cpu().numpy(), x.grad.cpu().numpy(), what="float64")

    # upstream factors 0 (an all-zero gradient, not NaN) and -1
    terms, grad = _run(img, tgt, "train", 0.0)
    assert (grad == 0.0).all()
    IC.judge(ref, "train", terms, grad, factor=0.0, what="factor 0")
    terms, grad = _run(img, tgt, "train", -1.0)
    IC.judge(ref, "train", terms, grad, factor=-1.0, what="factor -1")

    # all four weights 0: total exactly 0, gradient exactly 0, the terms still those of the pair
    x = img.to(DEV).requires_grad_(True)
    total, terms = L.fused_image_loss(x, tgt_d, l1_weight=0.0, l2_weight=0.0, ssim_weight=0.0, sobel_weight=0.0)
    total.backward()
    assert float(total) == 0.0 and float(terms[4]) == 0.0 and bool((x.grad == 0.0).all())
    assert (np.abs(terms[:4].cpu().numpy().astype(np.float64) - ref.t64[:4]) <= IC.term_bounds(ref)).all()

    # a side stream, the result read after stream.synchronize()
    side = torch.cuda.Stream(device=DEV)
    x = img.to(DEV).requires_grad_(True)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        total, terms = L.fused_image_loss(x, tgt_d, **_kw("train"))
        total.backward()
    side.synchronize()
    IC.judge(ref, "train", terms.cpu().numpy(), x.grad.cpu().numpy(), what="side stream")
    assert float(total) == float(terms[4])
