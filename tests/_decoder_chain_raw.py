"""TEST-ONLY caller of the fused decoder's *_chain entry points (include/ggd_raster.h: THE DECODER CHAINS): tests/_decoder_raw.py's
run() with the chain as an argument and a caller-provided attrs buffer.  Never imported by the product."""
import ctypes as C
from types import SimpleNamespace

import torch

import _decoder_raw as RAW
from gaussian_gan_decoder_amd import _capi
from gaussian_gan_decoder_amd import fused_decoder as FD

HID = RAW.HID


def unpack_wgrad(wg, chain):
    """wgrad [5, ggd_decoder_wgrad_floats() / 5] -> the 40 gradients by execution position, sliced to the chain's widths"""
    ch = FD._CHAIN_BY_ID[chain]
    grads = []
    for h in range(5):
        o = 0
        for nrow, ncol, r_used, c_used in ((HID, 64, HID, ch.in_features[h]), (HID, HID, HID, HID), (HID, HID, HID, HID),
                                           (16, HID, ch.out_dim[h], HID)):
            grads.append(wg[h, o:o + nrow * ncol].view(nrow, ncol)[:r_used, :c_used])
            o += nrow * ncol
            grads.append(wg[h, o:o + nrow][:r_used])
            o += nrow
    return grads


def run(mod, feats, pos, dattrs, precision="bf16", chunk=0, attrs_fill=None, entry="chain"):
    """forward_train / forward_hl, then backward_wgrad(_hl) with `chunk`, for the chain of `mod`'s type.  attrs_fill: what the
    attrs buffer holds before the forward (None: allocator leftovers, as in production; else a value, e.g. NaN).  entry: "chain"
    = the *_chain entry points; "plain" = the entry points without a chain (chain 0 only).  -> attrs, dout, dfeat, dinfo, zbuf,
    dzbuf, wg (raw), grads (40)."""
    hl = FD._check_precision(precision)
    chain = FD._check_decoder(mod).id
    assert entry == "chain" or chain == 0
    dev = feats.device
    n = pos.shape[0]
    feats, pos, dattrs = feats.contiguous().float(), pos.contiguous().float(), dattrs.contiguous().float()
    zbuf, dzbuf = RAW.planes(n, 0, device=dev), RAW.planes(n, 0, device=dev)
    cx = _capi.context_for(dev)
    lib = cx.lib
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    if entry == "chain":
        packed, packed_t = FD.device_pack(mod, hl=hl)
    else:   # the images through ggd_decoder_pack(_hl) itself
        params = [t.detach().float().contiguous() for head in FD._head_tensors(mod) for t in head]
        packed = torch.empty((lib.ggd_decoder_packed_hl_bytes() if hl else lib.ggd_decoder_packed_bytes(),), dtype=torch.uint8, device=dev)
        packed_t = torch.empty((lib.ggd_decoder_packed_t_hl_bytes() if hl else lib.ggd_decoder_packed_t_bytes(),), dtype=torch.uint8, device=dev)
        table = (C.c_void_p * 40)(*[t.data_ptr() for t in params])
        with torch.cuda.device(dev):
            cx.check((lib.ggd_decoder_pack_hl if hl else lib.ggd_decoder_pack)(cx.handle, st, table, p(packed), p(packed_t)))
    attrs = torch.empty((n, 16), dtype=torch.float32, device=dev)
    if attrs_fill is not None:
        attrs.fill_(attrs_fill)
    dout = torch.empty((5, n, 4), dtype=torch.float32, device=dev)
    dfeat = torch.empty((n, 32), dtype=torch.float32, device=dev)
    dinfo = torch.empty((n, 16), dtype=torch.float32, device=dev)
    wg = torch.zeros((5, lib.ggd_decoder_wgrad_floats() // 5), dtype=torch.float32, device=dev)
    sel = (chain,) if entry == "chain" else ()
    sfx = "_chain" if entry == "chain" else ""
    with torch.cuda.device(dev):
        fwd = getattr(lib, ("ggd_decoder_forward_hl" if hl else "ggd_decoder_forward_train") + sfx)
        cx.check(fwd(cx.handle, st, *sel, p(feats), p(pos), n, p(packed), p(attrs), p(zbuf)))
        bwd = getattr(lib, ("ggd_decoder_backward_wgrad_hl" if hl else "ggd_decoder_backward_wgrad") + sfx)
        cx.check(bwd(cx.handle, st, *sel, n, int(chunk), p(packed_t), p(attrs), p(dattrs), p(zbuf), p(dzbuf), p(dout), p(dfeat),
                     p(dinfo), p(feats), p(pos), p(wg)))
    torch.cuda.synchronize(dev)
    return SimpleNamespace(attrs=attrs, dout=dout, dfeat=dfeat, dinfo=dinfo, zbuf=zbuf, dzbuf=dzbuf, wg=wg, packed=packed, packed_t=packed_t,
                           grads=unpack_wgrad(wg, chain))
