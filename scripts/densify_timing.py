"""Device time of the density control (csrc/ggd_densify.hip) against the same work as a sequence of torch ops.
python scripts/densify_timing.py [--iters N] [--points P]

P rows (default 1 M), SH degree 0 and 3, inputs of tests/_densify_ref.make_case.  In one process, hipEvent pairs, medians over
--iters (default 20) runs after 3 warm-up runs:
  densify_and_prune                 GaussianModel.densify_and_prune (3 plan launches, 1 read-back, 1 gather launch)
  torch sequence                    _densify_ref.sequential on the same device tensors (clone cat, split cat, prune, prune)
  update_densification_stats        one launch
  torch statistics                  the loop's two masked lines (max_radii2D, then accum / denom)
The gather's traffic (source map + every parameter and moment read and written once) is set against 6.3 TB/s.
One JSON line per SH degree."""
import json
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from _densify_ref import NAMES, Rule, make_case, one_pass, sequential  # noqa: E402
from gaussian_gan_decoder_amd.gaussian_model import PARAM_GROUPS, GaussianModel  # noqa: E402

HBM_TBS = 6.3


def timed(fn, iters, warmup=3, setup=None):
    ms = []
    for it in range(warmup + iters):
        arg = setup() if setup else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(arg) if setup else fn(); b.record()
        b.synchronize()
        if it >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def measure(P, degree, iters, dev):
    M = (degree + 1) ** 2
    rule = Rule()
    case = make_case(P, M, 17 + degree, rule)
    _, counts = one_pass(case, rule)
    on_dev = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
    args = SimpleNamespace(percent_dense=rule.percent_dense, position_lr_init=0.00016, position_lr_final=0.0000016,
                           position_lr_delay_mult=0.01, position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05,
                           scaling_lr=0.005, rotation_lr=0.001)

    def fresh_model():
        pc = GaussianModel(degree)
        for name, attr in PARAM_GROUPS:
            setattr(pc, attr, torch.nn.Parameter(on_dev[name]))
        pc.spatial_lr_scale = 1.0
        pc.training_setup(args)
        for name, attr in PARAM_GROUPS:
            pc.optimizer.state[getattr(pc, attr)] = {"step": torch.tensor(1.0), "exp_avg": on_dev[name + ".m1"],
                                                     "exp_avg_sq": on_dev[name + ".m2"]}
        pc.xyz_gradient_accum, pc.denom = on_dev["accum"], on_dev["denom"]
        pc.max_radii2D = torch.zeros((P,), device=dev)
        return pc

    fused = timed(lambda pc: pc.densify_and_prune(rule.max_grad, rule.min_opacity, rule.extent, None, noise=on_dev["noise"]),
                  iters, setup=fresh_model)
    torch_ms = timed(lambda: sequential(on_dev, rule, dev), iters)
    # statistics
    gen = torch.Generator().manual_seed(1)
    vs = torch.zeros((P, 3), device=dev, requires_grad=True)
    vs.grad = (torch.randn((P, 3), generator=gen) * 1e-3).to(dev)
    radii = (torch.randint(0, 60, (P,), generator=gen) * (torch.rand((P,), generator=gen) < 0.6)).to(torch.int32).to(dev)
    pc = fresh_model()
    pc.xyz_gradient_accum, pc.denom = torch.zeros((P, 1), device=dev), torch.zeros((P, 1), device=dev)
    stats_fused = timed(lambda: pc.update_densification_stats(vs, radii), iters)
    accum, denom, max_radii = torch.zeros((P, 1), device=dev), torch.zeros((P, 1), device=dev), torch.zeros((P,), device=dev)

    def torch_stats():
        vis = radii > 0
        max_radii[vis] = torch.max(max_radii[vis], radii[vis])
        accum[vis] += torch.norm(vs.grad[vis, :2], dim=-1, keepdim=True)
        denom[vis] += 1
    stats_torch = timed(torch_stats, iters)
    # the gather alone: plan once, then time the emit launch through the C ABI
    import ctypes as C
    from gaussian_gan_decoder_amd import _capi
    cx, stream = _capi.context_and_stream(torch.device(dev))
    nbytes = cx.lib.ggd_densify_tmp_bytes(P)
    tmp = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    c4 = (C.c_int64 * 4)()
    vp = lambda t: C.c_void_p(t.data_ptr())
    cx.check(cx.lib.ggd_densify_plan(cx.handle, C.c_void_p(stream), P, vp(on_dev["accum"]), vp(on_dev["denom"]), vp(on_dev["scaling"]),
                                     vp(on_dev["opacity"]), rule.max_grad, rule.split_thr, rule.min_opacity, 0, rule.world_size,
                                     vp(tmp), nbytes, c4))
    new_P = int(c4[3])
    assert tuple(c4)[:3] == counts
    keys = [n + s for n in NAMES for s in ("", ".m1", ".m2")]
    outs = [torch.empty((new_P,) + tuple(on_dev[k].shape[1:]), device=dev) for k in keys]
    tin = (C.c_void_p * 18)(*[on_dev[k].data_ptr() for k in keys])
    tout = (C.c_void_p * 18)(*[t.data_ptr() for t in outs])
    emit = timed(lambda: cx.check(cx.lib.ggd_densify_emit(cx.handle, C.c_void_p(stream), P, new_P, M, tin, tout, vp(on_dev["noise"]),
                                                          vp(tmp), nbytes)), iters)
    plan = timed(lambda: cx.check(cx.lib.ggd_densify_plan(cx.handle, C.c_void_p(stream), P, vp(on_dev["accum"]), vp(on_dev["denom"]),
                                                          vp(on_dev["scaling"]), vp(on_dev["opacity"]), rule.max_grad, rule.split_thr,
                                                          rule.min_opacity, 0, rule.world_size, vp(tmp), nbytes, c4)), iters)
    W = 14 + 3 * (M - 1)
    moved = 4 * (3 * new_P * W + new_P * W + 2 * counts[0] * W) + 4 * new_P * 6   # writes + parameter reads + kept moments + map per group
    print(json.dumps(dict(P=P, sh_degree=degree, new_P=new_P, kept=counts[0], cloned=counts[1], split=counts[2],
                          densify_and_prune_ms=round(fused, 3), torch_sequence_ms=round(torch_ms, 3),
                          speedup=round(torch_ms / fused, 1), plan_ms=round(plan, 3), emit_ms=round(emit, 3),
                          emit_mb=round(moved / 1e6, 1), emit_tb_s=round(moved / emit / 1e9, 2),
                          emit_fraction_of_hbm=round(moved / emit / 1e9 / HBM_TBS, 2),
                          stats_ms=round(stats_fused, 4), torch_stats_ms=round(stats_torch, 4),
                          stats_speedup=round(stats_torch / stats_fused, 1))), flush=True)


def main():
    iters = max(20, int(sys.argv[sys.argv.index("--iters") + 1])) if "--iters" in sys.argv else 20
    P = int(sys.argv[sys.argv.index("--points") + 1]) if "--points" in sys.argv else 1_000_000
    if not torch.cuda.is_available():
        raise RuntimeError("densify_timing.py needs an MI355X: no HIP device visible")
    for degree in (0, 3):
        measure(P, degree, iters, "cuda:0")


if __name__ == "__main__":
    main()
