"""Stage times of the 3-nearest-neighbour call (ggd_knn3: box, Morton codes, sort, leaves, search) and its work measure.
python scripts/knn_timing.py [--iters N] [--sizes 100000,500000,...]

Inputs: 100 k / 1 M / 4 M uniform points in a cube and the decoder's own workload, 500 k iso-surface samples of a sphere
(target_sampler.sample_surface_points).  hipEvent pairs around every stage (ggd_knn3_stage, the stages of one iteration run
back to back in order) and around the whole call, 5 warm-up iterations, medians over --iters (default 30) runs.  At 100 k
the only other way to get the quantity from this repository's dependencies is timed too: a chunked torch.cdist + topk.
One JSON line per input."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gaussian_gan_decoder_amd import _capi, knn  # noqa: E402

STAGES = ("box", "codes", "sort", "leaves", "search")


def sphere_field(n):
    ax = (np.arange(n, dtype=np.float32) / np.float32(n)) - np.float32(0.5)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (np.float32(10.0) + np.float32(400.0) * (np.float32(0.3) - np.sqrt(x * x + y * y + z * z))).astype(np.float32)


def cdist_topk(p, chunk=2048):
    out = torch.empty(p.shape[0], device=p.device)
    for s in range(0, p.shape[0], chunk):
        d = torch.cdist(p[s:s + chunk], p)
        out[s:s + chunk] = (d.topk(4, dim=1, largest=False).values[:, 1:] ** 2).mean(dim=1)   # [0] is the point itself
    return out


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def measure(name, p, iters, brute):
    dev = p.device
    P = int(p.shape[0])
    cx, stream = _capi.context_and_stream(dev)
    lib = cx.lib
    nbytes = lib.ggd_knn_tmp_bytes(P)
    tmp = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mean = torch.empty(P, device=dev)
    vp = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(stream)

    def whole():
        cx.check(lib.ggd_knn3(cx.handle, st, vp(p), P, vp(mean), None, None, None, vp(tmp), nbytes))

    def stage(k):
        cx.check(lib.ggd_knn3_stage(cx.handle, st, vp(p), P, vp(mean), None, None, None, vp(tmp), nbytes, k))

    total = timed(whole, iters)
    ref = mean.clone()
    per = {k: [] for k in STAGES}
    for it in range(5 + iters):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
        ev[0].record()
        for k in range(len(STAGES)):
            stage(k)
            ev[k + 1].record()
        ev[-1].synchronize()
        if it >= 5:
            for k, n in enumerate(STAGES):
                per[n].append(ev[k].elapsed_time(ev[k + 1]))
    assert torch.equal(mean, ref)
    _, _, examined = knn.knn3(p, return_examined=True)
    L = knn.leaf_size()
    res = dict(input=name, P=P, leaf=L, call_ms=round(total, 4), stage_ms={k: round(statistics.median(v), 4) for k, v in per.items()},
               examined_per_point=round(int(examined.item()) / P, 1), examined_per_point_in_leaves=round(int(examined.item()) / P / L, 2),
               tmp_mib=round(nbytes / 2 ** 20, 1))
    if brute:
        res["cdist_topk_ms"] = round(timed(lambda: cdist_topk(p), 5, warmup=2), 3)
        rel = ((cdist_topk(p) - ref).abs() / ref.clamp_min(1e-20)).max().item()
        res["cdist_topk_max_rel_diff"] = float(f"{rel:.3e}")
    print(json.dumps(res), flush=True)


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 30
    sizes = [int(v) for v in sys.argv[sys.argv.index("--sizes") + 1].split(",")] if "--sizes" in sys.argv else [100_000, 500_000, 1_000_000, 4_000_000]
    if not torch.cuda.is_available():
        raise RuntimeError("knn_timing.py needs an MI355X: no HIP device visible")
    dev = torch.device("cuda:0")
    for P in sizes:
        if P == 500_000:
            from gaussian_gan_decoder_amd.target_sampler import sample_surface_points
            p, _ = sample_surface_points(torch.from_numpy(sphere_field(128)).to(dev), 10.0, P, 0.1, seed=7)
            name = "500k surface samples (sphere)"
        else:
            p = (torch.rand((P, 3), generator=torch.Generator().manual_seed(P)) - 0.5).to(dev)
            name = f"{P // 1000}k uniform cube"
        measure(name, p.contiguous(), max(20, iters), brute=(P == 100_000))


if __name__ == "__main__":
    main()
