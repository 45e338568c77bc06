"""TEST-ONLY caller of the fused decoder's C entry points (include/ggd_raster.h) through _capi, with caller-provided zbuf /
dzbuf: what FusedDecoderFn does, step by step, plus the forms Python never calls -- a given `chunk`, and the split pair
ggd_decoder_backward + ggd_decoder_wgrad.  Never imported by the product."""
import ctypes as C
from types import SimpleNamespace

import torch

from gaussian_gan_decoder_amd import _capi
from gaussian_gan_decoder_amd import fused_decoder as FD

HID = 128


def planes(n, fill=None, device="cuda:0"):
    """A zbuf / dzbuf: [5 heads][3 layers] planes of ceil(n / 16) blocks of 16 points x 128 16-bit values (blocked Z layout,
    csrc/ggd_mlp.hip), as int16; fill: None (allocator leftovers), 0, or -1 (every byte 0xFF: NaN as f16 and as bf16)."""
    shape = (5, 3, (n + 15) // 16 * 16, HID)
    assert 2 * shape[0] * shape[1] * shape[2] * shape[3] == _capi.load().ggd_decoder_zbuf_bytes(n)
    if fill is None:
        return torch.empty(shape, dtype=torch.int16, device=device)
    return torch.full(shape, fill, dtype=torch.int16, device=device)


def rows(buf):
    """[5,3,Npad,128] in the blocked layout block[k][g][j][8] -> [15, Npad, 128] with one row per POINT (its 128 values in
    the order of the layout's positions, not of the features: enough to compare runs and to tell rows apart)"""
    npad = buf.shape[2]
    return buf.reshape(15, npad // 16, 4, 4, 16, 8).permute(0, 1, 4, 2, 3, 5).reshape(15, npad, HID)


def unpack_wgrad(wg):
    """wgrad [5, ggd_decoder_wgrad_floats() / 5] -> the 40 gradients, with the slicing of FusedDecoderFn.backward"""
    grads = []
    for h in range(5):
        in_dim, od = 35 + FD._N_EXTRA[h], FD._OUT_DIM[h]
        o = 0
        for nrow, ncol, r_used, c_used in ((HID, 64, HID, in_dim), (HID, HID, HID, HID), (HID, HID, HID, HID), (16, HID, od, HID)):
            grads.append(wg[h, o:o + nrow * ncol].view(nrow, ncol)[:r_used, :c_used])
            o += nrow * ncol
            grads.append(wg[h, o:o + nrow][:r_used])
            o += nrow
    return grads


def run(mod, feats, pos, dattrs, precision="bf16", chunk=0, split=False, zbuf=None, dzbuf=None):
    """forward_train / forward_hl, then the backward + weight gradients of `precision`: ggd_decoder_backward_wgrad(_hl) with
    `chunk`, or (split, bf16 only) ggd_decoder_backward followed by ggd_decoder_wgrad.  -> attrs, dout, dfeat, dinfo, zbuf,
    dzbuf (the raw planes), grads (40)."""
    hl = FD._check_precision(precision)
    assert not (split and hl), "the reference-precision tier has no split form"
    dev = feats.device
    n = pos.shape[0]
    feats, pos, dattrs = feats.contiguous().float(), pos.contiguous().float(), dattrs.contiguous().float()
    zbuf = planes(n, device=dev) if zbuf is None else zbuf
    dzbuf = planes(n, device=dev) if dzbuf is None else dzbuf
    packed, packed_t = FD.device_pack(mod, hl=hl)
    cx = _capi.context_for(dev)
    lib = cx.lib
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    attrs = torch.empty((n, 16), dtype=torch.float32, device=dev)
    dout = torch.empty((5, n, 4), dtype=torch.float32, device=dev)
    dfeat = torch.empty((n, 32), dtype=torch.float32, device=dev)
    dinfo = torch.empty((n, 16), dtype=torch.float32, device=dev)
    wg = torch.zeros((5, lib.ggd_decoder_wgrad_floats() // 5), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        fwd = lib.ggd_decoder_forward_hl if hl else lib.ggd_decoder_forward_train
        cx.check(fwd(cx.handle, st, p(feats), p(pos), n, p(packed), p(attrs), p(zbuf)))
        if split:
            cx.check(lib.ggd_decoder_backward(cx.handle, st, n, p(packed_t), p(attrs), p(dattrs), p(zbuf), p(dzbuf), p(dout),
                                              p(dfeat), p(dinfo)))
            cx.check(lib.ggd_decoder_wgrad(cx.handle, st, n, p(zbuf), p(dzbuf), p(dout), p(feats), p(pos), p(attrs), p(wg)))
        else:
            bwd = lib.ggd_decoder_backward_wgrad_hl if hl else lib.ggd_decoder_backward_wgrad
            cx.check(bwd(cx.handle, st, n, int(chunk), p(packed_t), p(attrs), p(dattrs), p(zbuf), p(dzbuf), p(dout), p(dfeat),
                         p(dinfo), p(feats), p(pos), p(wg)))
    torch.cuda.synchronize(dev)
    return SimpleNamespace(attrs=attrs, dout=dout, dfeat=dfeat, dinfo=dinfo, zbuf=zbuf, dzbuf=dzbuf, grads=unpack_wgrad(wg))
