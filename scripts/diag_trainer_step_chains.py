"""python scripts/diag_trainer_step_chains.py  (one GPU) -- behind tests/test_decoder_chains_gpu.py::test_one_trainer_step and
DESIGN.md section 6r: why do the xyz head's tensors miss the flat relative-L2 bar?  For each decoder type and tier: per-tensor relative L2 of the
fused trainer's decoder gradients against the PyTorch trainer's, and -- at the fused trainer's OWN feats / pos / dattrs -- the
kernel's error and the tier restatement's deviation (dev) against the float64 restatement."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import _decoder_chain_ref as CR
from gaussian_gan_decoder_amd import fused_decoder as FD
from gaussian_gan_decoder_amd.train import DecoderTrainer, make_scene_batch
dev = torch.device("cuda:0")
BUMP = "--bump" in sys.argv
print("decoder as initialised" if not BUMP else "scale bias + 3.5, opacity bias + 1", flush=True)
cap = {}
orig = FD.FusedDecoderFn.backward
def spy(ctx, dattrs):
    cap["feats"], cap["pos"] = ctx.saved_tensors[0].clone(), ctx.saved_tensors[1].clone()
    cap["dattrs"] = dattrs.clone()
    out = orig(ctx, dattrs)
    cap["grads"] = [g.clone() for g in out[6:]]
    return out
FD.FusedDecoderFn.backward = staticmethod(spy)
def make(t, fused, prec):
    tr = DecoderTrainer(dev, n_scenes_total=2, plane_res=32, plane_channels=32, hidden_dim=128, image_size=64, seed=7,
                        perceptual_weight=0.0, backbone_params=0, decoder_type=t, fused_decoder=fused, decoder_precision=prec)
    if BUMP:   # --bump: larger, more opaque splats (what tests/test_train_step_gpu.py does so that a 64 x 64 image sees 2 000 points)
        with torch.no_grad():
            tr.decoder.scale_decoder.backbone[-1].bias += 3.5
            tr.decoder.opacity_decoder.backbone[-1].bias += 1.0
    return tr
def half(tr):
    tr.flat_grad.zero_()
    loss = tr.local_loss(make_scene_batch([0, 1], 2048, 64, dev, seed=0)); loss.backward(); torch.cuda.synchronize()
    return float(loss.detach())
for ci, t in enumerate(("sequential_reversed", "sequential", "parallel")):
    for prec in ("bf16", "fp32"):
        a, b = make(t, False, prec), make(t, True, prec)
        l0, l1 = half(a), half(b)
        names = {id(p): n for n, p in a.decoder.named_parameters()}
        off, rows = 0, []
        for p in a.params:
            k = p.numel()
            if id(p) in names:
                x, y = a.flat_grad[off:off + k], b.flat_grad[off:off + k]
                rows.append((float((x - y).norm() / x.norm()), names[id(p)]))
            off += k
        rows.sort(reverse=True)
        print(f"{t} {prec}: loss rel {abs(l1-l0)/abs(l0):.2e}; worst tensors vs PyTorch trainer: " + ", ".join(f"{n} {r:.3e}" for r, n in rows[:3]), flush=True)
        # the criterion at the trainer's own dattrs
        params64 = CR.module_params(b.decoder, ci, torch.float64)
        with torch.no_grad():
            ref = CR.decoder_chain_ref(ci, params64, cap["feats"].double(), cap["pos"].double(), cap["dattrs"].double())
            pre = CR.decoder_chain_ref(ci, params64, cap["feats"].double(), cap["pos"].double(), cap["dattrs"].double(), CR.TIERS[prec])
        pn = [n for n, _ in b.decoder.named_parameters()]
        worst = []
        for k in range(40):
            r = ref.grads[k]
            e = float((cap["grads"][k].double() - r).norm() / r.norm()); d = float((pre.grads[k] - r).norm() / r.norm())
            worst.append((e, d, pn[k]))
        worst.sort(reverse=True)
        print("    same dattrs, vs float64 restatement (kernel err L2, tier dev L2): " + ", ".join(f"{n} {e:.3e}/{d:.3e}" for e, d, n in worst[:3]), flush=True)
