"""CPU tests of the fused decoder's three chains: tests/_decoder_chain_ref.py, the yardstick of
tests/test_decoder_chains_gpu.py, is float64 autograd of SequentialDecoder / ParallelDecoder, is decoder_ref for chain 0 and
reproduces the reference-class fixtures; the Python front-ends take the chain from the module's type; the trainer's
decoder_type builds the right module and leaves the default untouched; the new kernel instances stay inside chain 0's
scratch, spill and LDS figures."""
import functools
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import _decoder_chain_ref as CR
import _decoder_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = {1: "forward_chain_decoder_fixture.npz", 2: "parallel_decoder_fixture.npz"}


@functools.lru_cache(maxsize=None)
def _case(chain, n):
    mod = CR.make_decoder(chain).double()
    feats, pos, dattrs = (t.double() for t in CR.make_inputs(n))
    return mod, feats, pos, dattrs, CR.decoder_chain_ref(chain, CR.module_params(mod, chain), feats, pos, dattrs)


def test_chain_table():
    c0, c1, c2 = CR.CHAINS
    assert c0.n_extra == (0, 3, 4, 8, 11) and c0.in_features == (35, 38, 39, 43, 46)
    assert c1.n_extra == (0, 3, 6, 10, 11) and c1.in_features == (35, 38, 41, 45, 46)
    assert c2.n_extra == (0,) * 5 and c2.in_features == (35,) * 5
    assert c1.heads == c2.heads == ("xyz_decoder", "scale_decoder", "rotation_decoder", "opacity_decoder", "color_decoder")
    assert c0.cols[:11] == list(range(11)) and c1.cols[:11] == [11, 12, 13, 8, 9, 10, 4, 5, 6, 7, 3]
    from gaussian_gan_decoder_amd import fused_decoder as FD
    for ch in CR.CHAINS:
        mine = FD._CHAINS[CR.module_class(ch.id)]
        assert (mine.id, mine.heads, mine.out_dim, mine.n_extra, mine.in_features) == \
            (ch.id, ch.heads, ch.od, ch.n_extra, ch.in_features)
        assert list(mine.cols) == (ch.cols[:11] if ch.chained else [])
    assert (FD._HEADS, FD._OUT_DIM, FD._N_EXTRA, FD._IN_FEATURES) == (R.HEADS, R.OD, R.A0, (35, 38, 39, 43, 46))


@pytest.mark.parametrize("n", [1, 33, 4099])
@pytest.mark.parametrize("chain", [1, 2])
def test_identity_hooks_are_float64_autograd_of_the_module(chain, n):
    """attrs, dfeat and all 40 parameter gradients of the restatement == autograd of the chain's module in float64 on plane
    features under the loss sum(attrs * dattrs): 1e-12 of each tensor's largest element (the bar of test_decoder_ref_host.py)."""
    mod, feats, pos, dattrs, ref = _case(chain, n)
    f = feats.clone().requires_grad_(True)
    for p in mod.parameters():
        p.grad = None
    o = mod(None, pos, features=f)
    attrs = torch.cat([o.color, o.opacity, o.rotation, o.scale, o.xyz], 1)
    (attrs * dattrs[:, :14]).sum().backward()

    def close(a, b, what):
        assert a.shape == b.shape, what
        err, scale = (a - b).abs().max().item(), b.abs().max().item()
        assert err <= 1e-12 * scale, (what, err, scale)
    close(ref.attrs[:, :14], attrs.detach(), "attrs")
    assert ref.attrs[:, 14:].abs().max().item() == 0
    close(ref.dfeat, f.grad, "dfeat")
    named = list(mod.named_parameters())
    assert len(named) == len(ref.grads) == 40
    assert [nm.split(".")[0] for nm, _ in named[::8]] == list(CR.CHAINS[chain].heads)
    for (name, p), g in zip(named, ref.grads):
        close(g, p.grad, name)


@pytest.mark.parametrize("tier", [None, "bf16", "fp32"])
def test_chain_0_is_decoder_ref_bit_for_bit(tier):
    mod = R.make_decoder().double()
    feats, pos, dattrs = (t.double() for t in R.make_inputs(257))
    t = R.IDENTITY if tier is None else R.TIERS[tier]
    a = R.decoder_ref(R.module_params(mod), feats, pos, dattrs, t)
    b = CR.decoder_chain_ref(0, CR.module_params(mod, 0), feats, pos, dattrs, t)
    for name in ("attrs", "dfeat", "dinfo", "dout"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert len(a.grads) == len(b.grads) == 40 and all(torch.equal(x, y) for x, y in zip(a.grads, b.grads))


def _fixture_module(chain):
    base = np.load(os.path.join(GOLDEN, "sequential_decoder_fixture.npz"))
    f = np.load(os.path.join(GOLDEN, FIXTURE[chain]))
    dec = CR.module_class(chain)()
    missing, unexpected = dec.load_state_dict({k[3:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("sd_")}, strict=False)
    assert not unexpected and not [m for m in missing if "decoder" in m], (missing, unexpected)
    return dec, torch.from_numpy(base["planes"]), torch.from_numpy(base["positions"]), f


@pytest.mark.parametrize("chain", [1, 2])
def test_restatement_reproduces_the_reference_class_fixtures(chain):
    """fp32 restatement on the fixture's plane features against the outputs of the REFERENCE's SequentialDecoder /
    ParallelDecoder: atol 2e-5, rtol 1e-5 (the bars tests/test_train_dp.py holds the modules to)."""
    from gaussian_gan_decoder_amd.decoder import triplane_mean
    dec, planes, pos, f = _fixture_module(chain)
    feats = triplane_mean(planes, pos, dec.box_warp, dec.plane_axes, dec.triplane_depth)
    with torch.no_grad():
        out = CR.decoder_chain_ref(chain, CR.module_params(dec, chain), feats, pos, torch.zeros(pos.shape[0], 16))
    for k, a in zip(("color", "opacity", "rotation", "scale", "xyz"), range(5)):
        np.testing.assert_allclose(out.attrs[:, R.A0[a]:R.A0[a] + R.OD[a]].numpy(), f[k], atol=2e-5, rtol=1e-5, err_msg=k)


def test_zero_gradient_patterns_give_exact_zeros_in_float64():
    """What tests/test_decoder_chains_gpu.py asserts as exact zeros on the device is a property of the operation: parallel chain,
    loss on colour only -> the other four heads' 32 gradients are exactly zero; sequential chain, loss on xyz only (the FIRST
    head) -> every later head's are; loss on colour only (the LAST head) -> all five heads receive gradient."""
    mod, feats, pos, dattrs, _ = _case(2, 257)
    out = CR.decoder_chain_ref(2, CR.module_params(mod, 2), feats, pos, CR.only(dattrs, 0))
    assert all(torch.count_nonzero(g).item() == 0 for g in out.grads[:32]) and all(torch.count_nonzero(g).item() > 0 for g in out.grads[32:])
    assert torch.count_nonzero(out.dinfo[:, 3:]).item() == 0
    mod, feats, pos, dattrs, _ = _case(1, 257)
    out = CR.decoder_chain_ref(1, CR.module_params(mod, 1), feats, pos, CR.only(dattrs, 4))
    assert all(torch.count_nonzero(g).item() > 0 for g in out.grads[:8]) and all(torch.count_nonzero(g).item() == 0 for g in out.grads[8:])
    out = CR.decoder_chain_ref(1, CR.module_params(mod, 1), feats, pos, CR.only(dattrs, 0))
    assert all(torch.count_nonzero(g).item() > 0 for g in out.grads)


# ---- the Python front-ends ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [1, 2])
def test_fused_decoder_constructs_on_the_cpu(native_lib, chain):
    """FusedDecoder(SequentialDecoder()) / FusedDecoder(ParallelDecoder()) on the CPU: the host statement of the 16-bit image,
    ggd_decoder_packed_bytes() bytes, heads in execution order; repack() follows the parameters."""
    from gaussian_gan_decoder_amd import fused_decoder as FD
    mod = CR.make_decoder(chain)
    fused = FD.FusedDecoder(mod)
    assert fused.chain.id == chain
    assert fused.packed.dtype == torch.uint8 and fused.packed.numel() == native_lib.ggd_decoder_packed_bytes()
    assert FD.pack_weights_t(mod).numel() == native_lib.ggd_decoder_packed_t_bytes()
    per = fused.packed.numel() // 5
    # slot 0 holds the chain's first head: xyz, whose W4 has 3 rows and whose W1 has 35 columns
    w1 = mod.xyz_decoder.backbone[0].weight.detach()
    w1f = torch.zeros(128, 64); w1f[:, :35] = w1
    want = FD._swizzle_rows(FD._permute_blocks(0.5 * w1f)).to(torch.float16).contiguous().view(torch.uint8).reshape(-1)
    assert torch.equal(fused.packed[:want.numel()], want)
    before = fused.packed.clone()
    with torch.no_grad():
        mod.color_decoder.backbone[6].bias.add_(1.0)     # the LAST head of chains 1, 2: the last bytes of the image
    fused.repack()
    assert torch.equal(fused.packed[:4 * per], before[:4 * per]) and not torch.equal(fused.packed[4 * per:], before[4 * per:])
    with pytest.raises(RuntimeError, match="move the decoder to the GPU"):
        FD.FusedDecoder(mod, precision="fp32")


def test_chain_0_host_images_are_the_earlier_formula(native_lib):
    """pack_weights / pack_weights_t of a SequentialDecoderReverse, byte for byte, against the formula they had before the chains
    (heads colour, opacity, rotation, scale, xyz; restated here)."""
    from gaussian_gan_decoder_amd import fused_decoder as FD
    mod = R.make_decoder()
    as_bytes = lambda t: t.contiguous().view(torch.uint8).reshape(-1)
    fwd, bwd = [], []
    for name in ("color_decoder", "opacity_decoder", "rotation_decoder", "scale_decoder", "xyz_decoder"):
        bb = getattr(mod, name).backbone
        w1, b1, w2, b2, w3, b3, w4, b4 = [t.detach().float() for k in (0, 2, 4, 6) for t in (bb[k].weight, bb[k].bias)]
        w1f = torch.zeros(128, 64); w1f[:, :w1.shape[1]] = w1
        w4f = torch.zeros(16, 128); w4f[:w4.shape[0]] = w4
        b4f = torch.zeros(16); b4f[:b4.shape[0]] = b4
        for w in (0.5 * w1f, 0.5 * w2, 0.5 * w3, w4f):
            fwd.append(as_bytes(FD._swizzle_rows(FD._permute_blocks(w)).clamp(-65504.0, 65504.0).to(torch.float16)))
        fwd.append(as_bytes(torch.cat([0.5 * b1, 0.5 * b2, 0.5 * b3, b4f])))
        w4t = torch.zeros(32, 128); w4t[:w4.shape[0]] = w4
        w4p = torch.zeros(128, FD.ROW4T); w4p[:, :32] = FD._permute_blocks(w4t.t().contiguous())
        bwd.append(as_bytes(w4p.to(torch.bfloat16)))
        for w in (w3, w2, w1f):
            bwd.append(as_bytes(FD._swizzle_rows(FD._permute_blocks(w.t().contiguous())).to(torch.bfloat16)))
    assert torch.equal(FD.pack_weights(mod), torch.cat(fwd))
    assert torch.equal(FD.pack_weights_t(mod), torch.cat(bwd))


def test_what_the_kernels_do_not_implement_still_raises():
    from gaussian_gan_decoder_amd import decoder as D
    from gaussian_gan_decoder_amd import fused_decoder as FD
    for cls in (D.SequentialDecoderReverse, D.SequentialDecoder, D.ParallelDecoder):
        with pytest.raises(ValueError, match="use_xyz_embedding"):
            FD.FusedDecoder(cls(use_xyz_embedding=True))
        with pytest.raises(ValueError, match="hidden_dim"):
            FD.FusedTrainDecoder(cls(hidden_dim=64))
        with pytest.raises(ValueError, match="first-layer widths"):
            FD.FusedDecoder(cls(plane_channels=16))

    class Foreign(D.SequentialDecoder):      # a subclass may reorder the heads: only the three types themselves are known
        pass
    for mod in (Foreign(), torch.nn.Linear(3, 3)):
        with pytest.raises(TypeError, match="SequentialDecoderReverse, SequentialDecoder and ParallelDecoder"):
            FD.FusedDecoder(mod)


def test_modules_take_gathered_features():
    """SequentialDecoder / ParallelDecoder .forward(features=...) == the call on the planes"""
    from gaussian_gan_decoder_amd.decoder import triplane_mean
    for chain in (1, 2):
        dec, planes, pos, _ = _fixture_module(chain)
        with torch.no_grad():
            a = dec(planes, pos)
            b = dec(None, pos, features=triplane_mean(planes, pos, dec.box_warp, dec.plane_axes, dec.triplane_depth))
        for k in ("xyz", "scale", "rotation", "opacity", "color"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k


# ---- the trainer -------------------------------------------------------------------------------------------------------------
def _trainer(**kw):
    from _cpu_render import render_simple_cpu
    from _torch_losses import image_loss_torch
    from gaussian_gan_decoder_amd.train import DecoderTrainer
    return DecoderTrainer("cpu", n_scenes_total=2, plane_res=8, image_size=16, render_fn=render_simple_cpu,
                          loss_fn=image_loss_torch, seed=5, **kw)


def test_trainer_decoder_type():
    from gaussian_gan_decoder_amd import decoder as D
    widths = lambda tr: tuple(getattr(tr.decoder, n).backbone[0].in_features
                              for n in ("xyz_decoder", "scale_decoder", "rotation_decoder", "opacity_decoder", "color_decoder"))
    tr = _trainer(decoder_type="sequential")
    assert type(tr.decoder) is D.SequentialDecoder and widths(tr) == (35, 38, 41, 45, 46)
    tr = _trainer(decoder_type="parallel")
    assert type(tr.decoder) is D.ParallelDecoder and widths(tr) == (35,) * 5
    tr = _trainer(decoder_type="sequential_reversed")
    assert type(tr.decoder) is D.SequentialDecoderReverse and widths(tr) == (46, 43, 39, 38, 35)
    with pytest.raises(ValueError, match="decoder_type"):
        _trainer(decoder_type="triplane_sr")


def test_default_trainer_is_unchanged():
    """No decoder_type: a SequentialDecoderReverse whose parameters are, bit for bit, those of one constructed after the same
    torch.manual_seed (what the trainer did before it had the option)."""
    from gaussian_gan_decoder_amd.decoder import SequentialDecoderReverse
    tr = _trainer()
    assert type(tr.decoder) is SequentialDecoderReverse and tr.decoder_type == "sequential_reversed"
    torch.manual_seed(5)
    want = SequentialDecoderReverse(32, 128)
    got = dict(tr.decoder.named_parameters())
    assert list(got) == [n for n, _ in want.named_parameters()]
    for n, p in want.named_parameters():
        assert torch.equal(got[n], p), n


# ---- the kernels' resources --------------------------------------------------------------------------------------------------
def test_new_chain_instances_stay_inside_chain_0s_resources(native_lib):
    """For every decoder kernel and tier, the chain-1 and chain-2 instances have no more scratch, no more spilled VGPRs and no
    more LDS than the chain-0 instance (read from the code objects in the built library, scripts/kernel_resources.py)."""
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec); spec.loader.exec_module(kr)
    from gaussian_gan_decoder_amd import _capi
    groups = {}
    for name, r in kr.kernel_resources(_capi.LIB_PATH).items():
        # demangled "decoder_x_kernel<1, true>" or, where the demangler does not know the 16-bit types, "..decoder_x_kernelILi1ELb1EE.."
        m = re.search(r"(decoder_(?:forward|backward|wgrad)(?:_hl)?_kernel)(?:<(\d)(?:, (true|false))?>|ILi(\d)E(?:Lb([01])E)?E)", name)
        if not m:
            continue
        chain = int(m.group(2) if m.group(2) is not None else m.group(4))
        store_z = {"true": 1, "false": 0, None: None}[m.group(3)] if m.group(2) is not None else (None if m.group(5) is None else int(m.group(5)))
        groups.setdefault((m.group(1), store_z), {})[chain] = r
    assert sorted(groups, key=str) == sorted([(f"decoder_{k}{t}_kernel", z) for t in ("", "_hl")
                                              for k, zs in (("forward", (0, 1)), ("backward", (None,)), ("wgrad", (None,)))
                                              for z in zs], key=str), sorted(groups, key=str)
    for key, inst in groups.items():
        assert sorted(inst) == [0, 1, 2], (key, sorted(inst))
        for chain in (1, 2):
            for fig in ("scratch", "vgpr_spill", "lds"):
                assert inst[chain][fig] <= inst[0][fig], (key, chain, fig, inst[chain], inst[0])
        if "_hl_" in key[0] and "wgrad" not in key[0]:      # these name v[248:255]: every instance owns the whole file
            assert all(r["vgpr"] == 256 and r["vgpr_spill"] <= 16 for r in inst.values()), (key, inst)
