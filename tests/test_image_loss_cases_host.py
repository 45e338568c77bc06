"""The image-loss edge table (tests/_image_loss_cases.py) proved sound from the reference alone, on the CPU: the ties it
promises are there and carry a zero L1 gradient in float64, the module's analytic a, b, c gradient is float64 autograd's, and
every bound that follows the float32 restatement's own deviation stays under a fixed cap, so that no tolerance can grow until it
hides a failure.  If a cap fails on another CPU, the case changes (seed or variant), never the cap."""
import numpy as np
import pytest
import torch

import _image_loss_cases as IC

NON_EQUAL = [k for k in IC.keys() if k[2] != "equal"]


def test_table_is_the_one_the_gpu_tests_expect():
    assert len(IC.SHAPES) == 13 and len(IC.keys()) == 52 and list(IC.WEIGHTS) == ["l1", "l2", "ssim", "sobel", "train"]
    for (H, W, v) in IC.keys():
        img, tgt = IC.case(H, W, v)
        assert img.shape == tgt.shape == (3, H, W) and img.dtype == tgt.dtype == torch.float32
        assert img.is_contiguous() and bool(torch.isfinite(img).all())
    img, tgt = IC.case(7, 1, "black")
    assert float(img.abs().max()) == 0.0 and float(tgt.abs().max()) == 0.0        # W // 2 == 0: an all-zero pair
    img, tgt = IC.case(70, 97, "over")
    assert float(img.min()) < 0.0 and float(img.max()) > 1.0 and float(tgt.min()) < -0.25 and float(tgt.max()) > 1.25
    img, tgt = IC.case(33, 31, "equal")
    assert torch.equal(img, tgt) and img.data_ptr() != tgt.data_ptr()
    assert float(IC.case(70, 97, "tex")[0].max()) > 1.0                           # not clamped
    # (70, 97): 3 x 4 tiles of 32, and tile (1, 1) keeps its 5-pixel halo inside the image
    assert -(-70 // 32) == 3 and -(-97 // 32) == 4 and 32 - 5 >= 0 and 64 + 5 <= 70 and 64 + 5 <= 97


@pytest.mark.parametrize("key", NON_EQUAL, ids=lambda k: f"{k[0]}x{k[1]}-{k[2]}")
def test_ties_are_there_and_have_a_zero_l1_gradient(key):
    """At least 20 % of the pixels of every case with H W >= 20 are ties (image == target); on every tie the float64 L1
    gradient (the reference's abs backward) is exactly 0, and off the ties it is +-1 / (3HW)."""
    img, tgt = IC.case(*key)
    tie = (img == tgt).numpy()
    H, W, _ = key
    if H * W >= 20:
        assert tie.mean() >= 0.20, tie.mean()
    _, g64 = IC.reference(key, "l1")
    assert (g64[tie] == 0.0).all()
    np.testing.assert_allclose(np.abs(g64[~tie]), 1.0 / (3 * H * W), rtol=1e-14)


@pytest.mark.parametrize("key", IC.keys(), ids=lambda k: f"{k[0]}x{k[1]}-{k[2]}")
def test_analytic_ssim_gradient_is_float64_autograd(key):
    """-1/(3HW) [G*a + 2x G*b + y G*c] against autograd of the restatement, to 1e-12 of the largest piece."""
    grad, piece = IC.ssim_pieces(*IC.case(*key))
    _, g64 = IC.reference(key, "ssim")
    assert (piece >= np.abs(grad) * (1 - 1e-12)).all()
    assert piece.max() > 0.0 or float(IC.case(*key)[0].abs().max()) == 0.0      # an all-zero pair has no pieces
    assert np.abs(grad - g64).max() <= 1e-12 * piece.max(), (np.abs(grad - g64).max(), piece.max())


@pytest.mark.parametrize("key", IC.keys(), ids=lambda k: f"{k[0]}x{k[1]}-{k[2]}")
def test_bounds_are_capped(key):
    """L1, L2, Sobel and the training weights: 4 dev32_grad <= 1e-5 max|g64| (the float32 restatement uses at most a quarter of
    the bar, so the bar rules alone).  1 - SSIM: the gradient bound <= 5e-5 max|g64|, the term bound <= 1e-6.  `equal`: L1,
    L2 and Sobel are exactly 0 in float32 and float64; the training weights' gradient there is the SSIM cancellation and follows
    its rule, which is capped against a real gradient of the same size: <= 5e-5 of the `tex` case's max|g64|."""
    H, W, variant = key
    equal = variant == "equal"
    for wname in IC.WEIGHTS:
        ref = IC._ref(*key, wname)
        gmax = float(np.abs(ref.g64).max())
        if wname in ("l1", "l2", "sobel"):
            assert 4.0 * ref.dev_grad <= 1e-5 * gmax, (wname, ref.dev_grad, gmax)
            if equal:
                k = list(IC.WEIGHTS).index(wname)
                assert ref.t64[k] == 0.0 and ref.dev_terms[k] == 0.0 and gmax == 0.0 and ref.dev_grad == 0.0
        elif equal:
            tex_gmax = float(np.abs(IC.reference((H, W, "tex"), wname)[1]).max())
            assert IC.grad_bound(ref, wname, IC.equal_piece_max(H, W)) <= 5e-5 * tex_gmax
        elif wname == "train":
            assert 4.0 * ref.dev_grad <= 1e-5 * gmax, (wname, ref.dev_grad, gmax)
        else:
            assert IC.grad_bound(ref, wname) <= 5e-5 * gmax, (IC.grad_bound(ref, wname), gmax)
        assert IC.term_bounds(ref)[2] <= 1e-6, IC.term_bounds(ref)


def test_float32_restatement_passes_its_own_rules():
    """The judge used on the kernel accepts the float32 restatement on every case and weight vector (a check of the judge and
    of the bounds, not of the kernel), and rejects an L1 sign(0) of +1, an L2 factor of 1.999 and a lost gradient element."""
    worst = {}
    for key in IC.keys():
        piece = IC.equal_piece_max(key[0], key[1]) if key[2] == "equal" else None
        for wname, w in IC.WEIGHTS.items():
            ref = IC._ref(*key, wname)
            x = IC.case(*key)[0].clone().requires_grad_(True)
            total, terms = IC.MR.masked_image_loss_torch(x, IC.case(*key)[1], *w)
            (-2.5 * total).backward()
            t5 = np.append(terms.detach().numpy(), np.float32(total.item()))
            r = IC.judge(ref, wname, t5, x.grad.numpy(), factor=-2.5, piece_max=piece, what=key)
            for n, v in r.items():
                worst[n] = max(worst.get(n, 0.0), v)
    print("\n  float32 restatement, worst error / bound: " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    key = (33, 31, "tex")
    img, tgt = IC.case(*key)
    n3 = float(img.numel())
    for wname, wrong in (("l1", np.where((img >= tgt).numpy(), 1.0, -1.0) / n3), ("l2", 1.999 * (img - tgt).double().numpy() / n3)):
        ref = IC._ref(*key, wname)
        t5 = np.append(ref.t64[:4], ref.t64[list(IC.WEIGHTS).index(wname)]).astype(np.float32)
        IC.judge(ref, wname, t5, ref.g64.astype(np.float32), what=key)
        with pytest.raises(AssertionError):
            IC.judge(ref, wname, t5, wrong.astype(np.float32), what=key)
        lost = ref.g64.astype(np.float32)
        lost[2, 32, 30] = np.nan
        with pytest.raises(AssertionError):
            IC.judge(ref, wname, t5, lost, what=key)
