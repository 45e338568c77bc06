"""Case tables of the teacher renderer's per-ray kernels (csrc/ggd_teacher.hip) at the sample counts and ray counts where the code
branches, and the constants of their bars.  CPU only: tests/test_teacher_render_cases_host.py proves every premise below on the
torch form and measures every constant again, tests/test_teacher_render_shapes_gpu.py runs the tables on the device.

Every case takes its planes, decoder, crop and axes from a fixture case (tests/_teacher_render_ref.py: T.case(name)), its rays
from that case's rays (row i is ray i % c.M) and its noise from torch.Generator().manual_seed(seed) on the CPU.

  table N   the union size n = Nc + Ni around one wave: tr_composite_kernel marches interval p = lane (set A) and p = 64 + lane
            (set B), takes `if (nm > 64)` for B's scan (nm = n - 1), chains the scans through lane 63 of A and splits the feature
            walk at (nm + 1) >> 1.  M = 9: three workgroups, the last with one live wave and three that recompute ray M - 1.
  table D   density extremes: the sigma entry of the last layer's bias shifted until the transmittance is gone inside set A
            ("opaque": B's weights come from the chained product alone, softplus takes z > 20) or every alpha is tiny ("empty").
  table M   ray counts around tr_clamp_kernel's stride of 1024: rows that miss the cropped region, and the call's smallest and
            largest sample depth each on ONE chosen ray, in the first trip of the stride loop ("front") or past it ("tail").
  table C   the public path: camera_rays at R = 23 for the fixture's two skewed cameras (M = 1058), drawn noise, images(),
            geometry().

`build(case)` gives a case's inputs, `reference(case)` the torch form's result on them, `deviations(case)` the worst distance of
that result's stages from the float64 restatement fed the SAME fp32 intermediates (all cached: do not modify).  MEASURED records
the worst deviation per table, stage and output; the accepted tolerance is twice that (the rule of _teacher_render_ref.py: two
fp32 evaluations may stand on opposite sides of the float64 value).  Nothing here comes from a run of the kernels."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

from gaussian_gan_decoder_amd import density, teacher
from gaussian_gan_decoder_amd.decoder import planes_channels_last
import _teacher_render_ref as T

RAY_START, RAY_END = 2.25, 3.3
STAGES = ("fine", "features", "weights", "depth")
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
CLAMP_STRIDE = 1024                  # tr_clamp_kernel: one workgroup of 1024 lanes (sixteen waves), i += 1024

# ---- table N ---------------------------------------------------------------------------------------------------------------------
N_FIELDS = ("pano_d3_sigmoid_48_48", "eg3d_64_64")          # crop on, D = 3; no crop, D = 0
N_RAYS = 9
N_COUNTS = {(4, 0): 3, (4, 1): 4, (5, 2): 6, (4, 64): 67,
            (32, 32): 63, (7, 57): 63, (57, 7): 63, (64, 0): 63,            # lane 63 of set A idle
            (33, 32): 64, (64, 1): 64,                                      # set A full, set B empty, the branch not taken
            (33, 33): 65, (64, 2): 65,                                      # one interval in set B
            (63, 64): 126, (64, 63): 126, (64, 64): 127}                    # (Nc, Ni) -> nm
AROUND_THE_WAVE = (63, 64, 65)

# ---- table D ---------------------------------------------------------------------------------------------------------------------
D_FIELD = "pano_d3_sigmoid_48_48"
D_COUNTS = ((33, 33), (48, 48))
# added to the sigma entry of the second layer's effective bias.  Chosen on the CPU (test_teacher_render_cases_host.py asserts
# each premise): the field's own sigma spans -0.9 .. 0.7 over these rays, so +60 puts every marched sigma_mid - 1 above softplus'
# threshold of 20 and leaves less than 1e-10 of any ray's weight to the intervals of set B; -10 makes every alpha about 1e-6.
# Not smaller: the restatement forms alpha as 1 - exp(-x) in float64, whose absolute error of 1e-16 must stay below 1e-9 of alpha
# for its depth (a ratio of two sums of alphas) to be the yardstick.
D_SHIFTS = {"opaque": 60.0, "empty": -10.0}
OPAQUE_AT_LEAST, EMPTY_AT_MOST = 0.999, 1e-4                # of the torch form's largest weight sum

# ---- table M ---------------------------------------------------------------------------------------------------------------------
M_FIELD = "pano_d1_lrelu_white_8_5"
MISS_ORIGIN, MISS_DIR = (5.0, 0.0, 2.7), (0.0, 0.0, -1.0)   # x = 5 all along the ray: every sample cropped
# (M, Nc, Ni, placement, r_lo, r_hi).  "front": both extrema in the first trip of the clamp's stride loop; "tail": both past row
# 1024 and in different waves of the clamp workgroup (wave = (row % 1024) >> 6), which needs M >= 1024 + 65; "row1024": M = 1025
# has ONE row past the first trip, row 1024, which is also a miss -- its samples still count in the call's depth range, so both
# extrema sit on it: the only way the second trip can show at that M.
M_ROWS = [(1023, 8, 5, "front", 37, 700), (1024, 8, 5, "front", 37, 700), (1025, 8, 5, "front", 37, 700),
          (1025, 8, 5, "row1024", 1024, 1024), (2049, 8, 5, "front", 37, 700), (2049, 8, 5, "tail", 1124, 1924),
          (4099, 8, 5, "front", 37, 700), (4099, 8, 5, "tail", 2118, 4097),
          (1025, 48, 48, "front", 37, 700), (1025, 48, 48, "row1024", 1024, 1024)]

# ---- table C ---------------------------------------------------------------------------------------------------------------------
C_FIELD = "pano_d3_sigmoid_48_48"
C_RESOLUTION = 23                                           # 2 cameras x 23 x 23 = 1058 rays

# seeds: the case's place in its table; + 1 wherever the torch form on the CPU puts a fine sample within T.NEAR_CROP of the crop
# limit (the stage checks leave no ray out, so the inputs must not need it), one at a time until it shows none.  The M = 1025
# cases at 48 + 48 needed many steps: several of the 25 fixture rays run almost along the crop planes (|x| or |z| within 1e-3 of
# the limit over their whole length), so about five of their 49 200 fine samples land that close under a typical seed.
SEED_BASE = {"N": 1000, "D": 2000, "M": 3000, "C": 4000}
SEED_MOVED = {"M-1023-8+5-front": 1, "M-1025-8+5-row1024": 1, "M-2049-8+5-front": 1, "M-4099-8+5-front": 1,
              "M-1025-48+48-front": 71, "M-1025-48+48-row1024": 70, "C-R23-48+48": 4}     # case id -> how far its seed was moved up


def _case(table, index, cid, field, M, Nc, Ni, **more):
    a = dict(id=cid, table=table, field=field, M=M, Nc=Nc, Ni=Ni, nm=Nc + Ni - 1, seed=SEED_BASE[table] + index + SEED_MOVED.get(cid, 0),
             shift=0.0, kind=None, placement=None, r_lo=None, r_hi=None, miss=())
    a.update(more)
    return SimpleNamespace(**a)


def _miss_rows(M):
    return tuple(sorted({r for r in (0, 1023, 1024, M - 1) if r < M}))


TABLE_N = [_case("N", i, f"N-{f.split('_')[0]}-{Nc}+{Ni}", f, N_RAYS, Nc, Ni)
           for i, (f, (Nc, Ni)) in enumerate((f, k) for f in N_FIELDS for k in N_COUNTS)]
TABLE_D = [_case("D", i, f"D-{kind}-{Nc}+{Ni}", D_FIELD, N_RAYS, Nc, Ni, kind=kind, shift=D_SHIFTS[kind])
           for i, (kind, (Nc, Ni)) in enumerate((k, c) for k in D_SHIFTS for c in D_COUNTS)]
TABLE_M = [_case("M", i, f"M-{M}-{Nc}+{Ni}-{pl}", M_FIELD, M, Nc, Ni, placement=pl, r_lo=lo, r_hi=hi, miss=_miss_rows(M))
           for i, (M, Nc, Ni, pl, lo, hi) in enumerate(M_ROWS)]
TABLE_C = [_case("C", 0, f"C-R{C_RESOLUTION}-48+48", C_FIELD, 2 * C_RESOLUTION ** 2, 48, 48)]
TABLES = {"N": TABLE_N, "D": TABLE_D, "M": TABLE_M, "C": TABLE_C}
ALL = TABLE_N + TABLE_D + TABLE_M + TABLE_C
BY_ID = {c.id: c for c in ALL}

# worst |torch form on the CPU - float64 restatement fed its own fp32 intermediates| per table (absolute); the host test measures
# each again and asserts measured <= recorded <= 1.01 * measured (each is rounded up by about half a per cent)
MEASURED = {
    "N": SimpleNamespace(fine=3.97e-7, features=2.07e-7, weights=1.93e-7, depth=5.61e-7),
    "D": SimpleNamespace(fine=7.63e-7, features=2.27e-7, weights=1.222e-7, depth=6.43e-7),
    "M": SimpleNamespace(fine=9.24e-7, features=6.44e-7, weights=1.012e-7, depth=7.98e-7),
    "C": SimpleNamespace(fine=4.33e-7, features=7.79e-8, weights=9.22e-8, depth=7.26e-7),
}
TOL = {t: SimpleNamespace(**{k: 2.0 * v for k, v in vars(m).items()}) for t, m in MEASURED.items()}


def ids(cases):
    return [c.id for c in cases]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field(name, shift=0.0):
    """(fixture case, channel-last planes, OSGWeights with the sigma bias moved by shift) on the CPU"""
    c = T.case(name)
    w = density.osg_weights(c.decoder)
    if shift:
        b2 = w.b2.clone()
        b2[0] += shift
        w = density.OSGWeights(w.w1, w.b1, w.w2, b2, w.activation)
    return c, planes_channels_last(c.planes, c.D or None), w


def cameras():
    return torch.from_numpy(T.FIX["rays_cam2world"]), torch.from_numpy(T.FIX["rays_intrinsics"])


def draw(case, M, generator):
    """the two draws in render_teacher's order, on the generator's device"""
    dev = generator.device
    return (torch.rand((M, case.Nc), device=dev, generator=generator), torch.rand((M, case.Ni), device=dev, generator=generator))


@functools.lru_cache(maxsize=None)
def _build(cid):
    case = BY_ID[cid]
    c, cl, w = field(case.field, case.shift)
    kw = dict(T.render_kwargs(c), ray_start=RAY_START, ray_end=RAY_END, depth_resolution=case.Nc,
              depth_resolution_importance=case.Ni)
    if case.table == "C":
        o, d = teacher.camera_rays(*cameras(), C_RESOLUTION)
    else:
        idx = torch.arange(case.M) % c.M
        o, d = torch.from_numpy(c.origins)[idx].clone(), torch.from_numpy(c.dirs)[idx].clone()
    uc, uf = draw(case, case.M, torch.Generator().manual_seed(case.seed))
    if case.table == "M":
        rows = list(case.miss)
        o[rows], d[rows] = torch.tensor(MISS_ORIGIN), torch.tensor(MISS_DIR)
        uc[:, 0] = 0.1 + 0.8 * uc[:, 0]                      # every first draw >= 0.1, every last <= 0.9 ...
        uc[:, -1] = 0.9 * uc[:, -1]
        uc[case.r_lo, 0] = 0.0                               # ... but the chosen rays': the call's smallest and largest sample depth
        uc[case.r_hi, -1] = BELOW_ONE
    return SimpleNamespace(case=case, c=c, planes_cl=cl, weights=w, origins=o.contiguous(), dirs=d.contiguous(), u_coarse=uc,
                           u_fine=uf, kwargs=kw, white_back=c.white_back, lim=T.crop_limit(c))


def build(case):
    """the inputs of a case as CPU tensors (cached: do not modify)"""
    return _build(case.id)


@functools.lru_cache(maxsize=None)
def _reference(cid):
    b = _build(cid)
    return teacher.render_teacher_torch(b.planes_cl, b.weights, b.origins, b.dirs, noise=(b.u_coarse, b.u_fine), return_samples=True,
                                        **b.kwargs)


def reference(case):
    """render_teacher_torch on the case's CPU tensors, with its samples (cached: do not modify)"""
    return _reference(case.id)


# ---- the stage checks, for the torch form here and for the kernels in the GPU file ------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy()


def union(s):
    return (np.concatenate([_np(s.depths_coarse), _np(s.depths_fine)], 1), np.concatenate([_np(s.sigma_coarse), _np(s.sigma_fine)], 1),
            np.concatenate([_np(s.rgb_coarse), _np(s.rgb_fine)], 1))


def stage_deviations(out, u_fine, white_back):
    """an implementation's result with its samples -> (worst |result - float64 restatement fed the result's own fp32 samples| for
    the fine depths, features, weights and depth, every ray; the restatement's composite with the clamp bounds lo, hi)"""
    s = out.samples
    dev = dict(fine=0.0)
    if s.depths_fine.shape[1]:
        dev["fine"] = T.worst(_np(s.depths_fine), T.importance(_np(s.depths_coarse), _np(s.sigma_coarse), _np(u_fine)))
    want = T.composite(*union(s), white_back)
    for k in STAGES[1:]:
        dev[k] = T.worst(_np(getattr(out, k)), getattr(want, k))
    return dev, want


@functools.lru_cache(maxsize=None)
def _deviations(cid):
    b = _build(cid)
    return stage_deviations(_reference(cid), b.u_fine, b.white_back)[0]


def deviations(case):
    return _deviations(case.id)


def near_crop(case, coords_fine):
    """rays of the case with a fine sample within T.NEAR_CROP of the crop limit"""
    return T.near_crop_rays(build(case).c, _np(coords_fine))


def clamp_wave(row):
    return (row % CLAMP_STRIDE) >> 6
