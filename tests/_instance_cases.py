"""Case tables that reach every depth / alpha (AUX) and anti-aliasing (AA) kernel instance by construction.  CPU only:
tests/test_instance_cases_host.py proves the tables sound against the oracle, tests/test_instances_gpu.py runs them.

A case is a dict: id, table, scene (a key of SCENES, or None for table C), feature ("aa", "aux" or "aux+aa"), options
{exp_mode, cull, binning, split, fold, msd}, raw (bool) and, for table C, seed.  `inputs(case)` builds the activated inputs,
`reference(case)` the CPU oracle forward (at float32(o_eff) for an AA case) with its fragile-pixel mask; both are cached
and must not be modified.  The dispatch rules of the launchers are restated at the bottom as functions of a case."""
from __future__ import annotations

import functools

import numpy as np
import torch

import _antialias_ref as AA
from _util import adversarial_inputs, run_oracle, scene_inputs

DEFAULTS = dict(exp_mode=3, cull=1, binning=1, split=1, fold=1, msd=1)

# ---- table A: the blend instances.  7 x 5 and 5 x 7 tiles (no multiple of 8, half a tile at the edge); both scenes reach the
# T < 1e-4 early stop and hold Gaussians whose o_eff falls under 1/255
# ---- table B: the per-Gaussian kernel forms (plain: M = 1 or precomputed colours; _vec: M in {4, 8, 12, 16}; _staged: other M)
_B = dict(size=64, width=64, height=48, lsm=-4.5, P=2000)
SCENES = {
    "A1": lambda: scene_inputs(P=3000, size=104, width=104, height=72, kind="shell", lsm=-4.6, seed=61),
    "A2": lambda: scene_inputs(P=4000, size=104, width=72, height=104, kind="cube", lsm=-4.2, seed=62),
    "M1": lambda: scene_inputs(**_B, seed=63),
    "M4": lambda: scene_inputs(**_B, seed=64, sh_degree=1),
    "M9": lambda: scene_inputs(**_B, seed=65, sh_degree=2),
    "M16": lambda: scene_inputs(**_B, seed=66, sh_degree=3),
    "deg1-M16": lambda: scene_inputs(**_B, seed=67, sh_degree=1, sh_M=16),
    "colors": lambda: scene_inputs(**_B, seed=68, use_colors=True),
    "cov-M9": lambda: scene_inputs(**_B, kind="shell", seed=69, sh_degree=2, use_cov=True),
    # two workgroups of the per-Gaussian kernels, the second holding one Gaussian
    "P257-M9": lambda: scene_inputs(P=257, size=33, width=17, height=33, lsm=-3.5, seed=70, sh_degree=2),
    "adversarial": adversarial_inputs,
}
B_SCENES = [k for k in SCENES if k not in ("A1", "A2")]
# the raw-attribute runs need scales and rotations to activate; the adversarial scene (a zero quaternion, zero / full opacity:
# no logit) is left out
B_RAW_SCENES = [k for k in B_SCENES if k not in ("cov-M9", "adversarial")]


def _table_a():
    out = []
    for scene in ("A1", "A2"):
        for em in (0, 1, 2, 3):
            for cull in (0, 1):
                for feature in ("aux", "aux+aa"):
                    split = 3 if len(out) % 2 else 1     # every second case: the aux backward must ignore the option
                    out.append(dict(id=f"{scene}-exp{em}-cull{cull}-{feature}" + ("-split3" if split == 3 else ""), table="A",
                                    scene=scene, feature=feature, raw=False,
                                    options=dict(DEFAULTS, exp_mode=em, cull=cull, split=split)))
    return out


def _table_b():
    out = [dict(id=f"{scene}-{feature}", table="B", scene=scene, feature=feature, raw=False, options=dict(DEFAULTS))
           for scene in B_SCENES for feature in ("aa", "aux", "aux+aa")]
    out += [dict(id=f"{scene}-{feature}-raw", table="B", scene=scene, feature=feature, raw=True, options=dict(DEFAULTS))
            for scene in B_RAW_SCENES for feature in ("aa", "aux", "aux+aa")]
    return out


# ---- table C: the seeded fuzz -- _case(seed) of tests/test_fuzz_gpu.py with RandomState(5000 + seed), two more shapes, the feature
# from the seed, no blend-split draw and no pipeline branch (FramePipeline.submit has no depth / alpha keyword)
C_SHAPES = [(64, 64), (100, 52), (17, 33), (256, 144), (1, 1), (16, 16), (1100, 48), (40, 1090), (333, 333), (1040, 80),
            (8, 8), (15, 90)]
C_FEATURES = ("aux", "aa", "aux+aa")


@functools.lru_cache(maxsize=None)
def _fuzz(seed):
    rng = np.random.RandomState(5000 + seed)
    W, H = C_SHAPES[rng.randint(len(C_SHAPES))]
    P = int(rng.choice([1, 7, 64, 300, 2000, 6000]))
    deg = int(rng.randint(0, 4))
    M = int(rng.choice([(deg + 1) ** 2, 16])) if deg > 0 else 1
    use_colors = bool(rng.rand() < 0.2)
    use_cov = bool(rng.rand() < 0.2)
    d = scene_inputs(P=P, size=max(W, H), kind=str(rng.choice(["cube", "shell"])), seed=seed, sh_degree=0 if use_colors else deg,
                     sh_M=None if use_colors else M, use_colors=use_colors, use_cov=use_cov, lsm=float(rng.uniform(-6.5, -3.0)),
                     fov_deg=float(rng.uniform(6.0, 20.0)), width=W, height=H, scale_modifier=float(rng.choice([1.0, 0.7, 1.6])))
    opts = dict(DEFAULTS, binning=int(rng.choice([0, 1, 2, 3])), cull=int(rng.rand() < 0.8), exp_mode=int(rng.choice([0, 2, 3, 3])),
                fold=int(rng.rand() < 0.6), msd=int(rng.rand() < 0.7))
    raw = bool(rng.rand() < 0.25) if d["scales"] is not None else False
    return d, opts, raw


def fuzz_case(seed):
    d, opts, raw = _fuzz(seed)
    feature = C_FEATURES[seed % 3]
    M = 0 if d["shs"] is None else d["shs"].shape[1]
    what = f"seed{seed}-{d['W']}x{d['H']}-P{d['P']}-M{M}" + ("-cov" if d["cov3D_precomp"] is not None else "")
    what += f"-{feature}-exp{opts['exp_mode']}-cull{opts['cull']}-bin{opts['binning']}-fold{opts['fold']}-msd{opts['msd']}"
    return dict(id=what + ("-raw" if raw else ""), table="C", scene=None, seed=seed, feature=feature, raw=raw, options=opts)


# The first 96 seeds, in order from 0, whose fragile-pixel and fragile-Gaussian counts on the CPU oracle are at most half of each
# cap (`fragile_counts` against `caps`; 25, 91 and 93 are not).  tests/test_instance_cases_host.py asserts that of every kept seed
# and re-derives the list.  Chosen from the oracle alone, never from a GPU outcome.
C_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23,
           24, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48,
           49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72,
           73, 74, 75, 76, 77, 78, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 90, 92, 94, 95, 96, 97, 98)

TABLE_A = _table_a()
TABLE_B = _table_b()


def table_c():
    return [fuzz_case(s) for s in C_SEEDS]


def has_aa(case):
    return "aa" in case["feature"]


def has_aux(case):
    return "aux" in case["feature"]


def inputs(case):
    """the activated inputs of a case (cached: do not modify)"""
    return _scene(case["scene"]) if case["scene"] is not None else _fuzz(case["seed"])[0]


@functools.lru_cache(maxsize=None)
def _scene(name):
    return SCENES[name]()


def raw_inputs(d):
    """d with the opacities and scales before their activations (logit, log), as the raw-attribute tests build them"""
    return dict(d, opacities=torch.logit(d["opacities"].double()).float().contiguous(), scales=torch.log(d["scales"]).contiguous())


# A raw-attribute run blends records that differ from the activated run's by the rounding of the activations, not by an ulp of
# exp(): the scales go through log (stored in fp32: half an ulp of |log s| < 16, 2^-21 = 4.8e-7) and back through the kernel's
# expf (<= 2 ulps, 2.4e-7), so s moves by up to 7.2e-7 of itself, the covariance (a sum of s_k^2 terms) and with it the power
# -1/2 d^T conic d by up to 1.45e-6 of itself; at the alpha floor the power is ln(1 / (255 o)) >= -5.54, so alpha moves by up to
# 8e-6 of itself, plus 2e-7 for sigmoid(logit(o)).  The oracle's fragile-pixel mask with that window (1e-5 instead of the 1e-6
# that covers exp()) names every pixel where the two runs may blend another set of records.
RAW_WINDOW = 1e-5


def raw_fragile_pixels(case):
    """bool[H, W]: the oracle's fragile pixels of a raw-attribute case at RAW_WINDOW (cached: do not modify)"""
    return _raw_fragile(case["scene"], case.get("seed"), has_aa(case))


@functools.lru_cache(maxsize=None)
def _raw_fragile(scene, seed, aa):
    from oracle import ggd_oracle as O
    return O.fragile_pixels(_reference(scene, seed, aa)["o"], window=RAW_WINDOW)


COND_MAX = 1e3   # (tests/test_antialiasing_gpu.py: beyond it the fp32 h is not pinned by the formula)


def reference(case):
    """dict(d, o, frag, cond): the inputs the oracle ran on (for an AA case: the opacities replaced by float32(o_eff)), its
    forward, its fragile-pixel mask (unchecked: the caps are the host test's) and the largest conditioning of h over the
    visible Gaussians (0 without AA).  Cached per (scene or seed, AA): do not modify."""
    return _reference(case["scene"], case.get("seed"), has_aa(case))


@functools.lru_cache(maxsize=None)
def _reference(scene, seed, aa):
    from oracle import ggd_oracle as O
    d = _scene(scene) if scene is not None else _fuzz(seed)[0]
    cond = None
    if aa:
        _, cond = AA.h_and_conditioning(d)
        oe = torch.from_numpy(AA.o_eff(d).astype(np.float32)).reshape(d["opacities"].shape).contiguous()
        d = dict(d, opacities=oe)
    o = run_oracle(d)
    cond_max = float(cond[o["radii"] > 0].max(initial=0.0)) if aa else 0.0
    return dict(d=d, o=o, frag=O.fragile_pixels(o), cond=cond_max)


GRAD_SEED = 7


def upstream_gradients(H, W, frag=None, seed=GRAD_SEED):
    """N(0, 1) upstream gradients (colour [3, H, W], depth [1, H, W], alpha [1, H, W]) in the draw order of the depth / alpha and
    anti-aliasing tests' _grads, zero on the pixels of the bool mask `frag`"""
    gen = torch.Generator().manual_seed(seed)
    g = torch.randn(3, H, W, generator=gen)
    gD, gA = torch.randn(1, H, W, generator=gen), torch.randn(1, H, W, generator=gen)
    if frag is not None:
        m = torch.from_numpy(frag)
        g[:, m] = 0.0; gD[:, m] = 0.0; gA[:, m] = 0.0
    return g, gD, gA


def fragile_counts(case):
    """(fragile pixels, fragile Gaussians) of a case from the oracle alone: its fragile-pixel mask, and backward_ref64 -- colour
    and the depth / alpha pseudo-colour -- on the oracle's own final_T / n_contrib / lists"""
    return _fragile_counts(case["scene"], case.get("seed"), has_aa(case))


@functools.lru_cache(maxsize=None)
def _fragile_counts(scene, seed, aa):
    from oracle import ggd_oracle as O
    from _depth_alpha_ref import pseudo_rgb
    r = _reference(scene, seed, aa)
    o = r["o"]
    g, gD, gA = upstream_gradients(o["H"], o["W"], r["frag"])
    _, _, frag = O.backward_ref64(o, g.numpy())
    rgb = pseudo_rgb(o)
    g_aux = np.stack([gD.numpy()[0], gA.numpy()[0], np.zeros((o["H"], o["W"]), np.float32)])
    _, _, frag_a = O.backward_ref64(dict(o, rgb=rgb, bg=np.zeros(3, np.float32), colors_precomp=rgb), g_aux)
    return int(r["frag"].sum()), int((np.maximum(frag, frag_a) > 0).sum())


def caps(case):
    """half of the caps the helpers assert (fragile_pixels: 2 + W H // 5000; check_gradients: max(4, P // 1000)): met by the
    reference alone, so that a GPU run has the other half as its margin"""
    d = inputs(case)
    return (2 + d["W"] * d["H"] // 5000) // 2, max(4, d["P"] // 1000) // 2


# ---- the launchers' dispatch rules, restated (csrc/ggd_blend.hip::ggd_launch_blend / ggd_launch_blend_backward,
# csrc/ggd_preprocess_bwd.hip::ggd_launch_preprocess_backward, csrc/ggd_preprocess.hip::ggd_launch_preprocess)
def _b(v):
    return "true" if v else "false"


def _layout(case):
    d = inputs(case)
    M = 0 if d["shs"] is None else int(d["shs"].shape[1])
    staged = d["colors_precomp"] is None and M > 1
    shvec = staged and M <= 16 and (3 * M) % 4 == 0
    return staged, shvec


def forward_blend_instance(case):
    """the forward blend kernel of a case, None without the depth / alpha maps"""
    if not has_aux(case):
        return None
    em = case["options"]["exp_mode"]
    return f"blend_forward_kernel<{1 if em == 3 else em}, {_b(case['options']['cull'])}, false, true>"


def backward_blend_instance(case):
    if not has_aux(case):
        return None
    return f"blend_backward_quarter_kernel<{case['options']['exp_mode']}, {_b(case['options']['cull'])}, false, true>"


def preprocess_backward_instance(case):
    staged, shvec = _layout(case)
    aa, aux = _b(has_aa(case)), _b(has_aux(case))
    if shvec:
        return f"preprocess_backward_vec_kernel<{aa}, {aux}>"
    if staged:
        return f"preprocess_backward_staged_kernel<false, {aa}, {aux}>"
    return f"preprocess_backward_kernel<{aa}, {aux}>"


def preprocess_instances(case):
    """the forward per-Gaussian kernels of a case's two frames: the first (exact two-call path) is never folded, the second
    (single call) is where the option is on and a tile-binning path runs"""
    _, shvec = _layout(case)
    folded = case["options"]["fold"] != 0 and case["options"]["binning"] != 0
    return {f"preprocess_kernel<{_b(shvec)}, {_b(fo)}, {_b(has_aa(case))}>" for fo in {False, folded}}
