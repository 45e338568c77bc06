"""Case tables that reach every kernel instance with a `raw_attributes` branch.  CPU only:
tests/test_raw_cases_host.py proves the tables sound against the oracle and measures the constants below,
tests/test_raw_instances_gpu.py runs them against the float64 reference of tests/_raw_ref.py.

A case is a dict: id, table, scene (a key of _instance_cases.SCENES; None for table V), feature ("plain", "aa", "aux" or "aux+aa"),
edge (bool: the first rows set by hand), absgrad (bool) and options (the context options, _instance_cases.DEFAULTS).
`reference(case)` holds the raw inputs, their float64 activations, the oracle forward and its fragile-pixel mask at RAW_WINDOW;
cached, not to be modified."""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

import _antialias_ref as AA
import _camera_grad_ref as CR
import _instance_cases as IC
import _raw_ref as RR
from _util import KAPPA, run_oracle

FEATURES = ("plain", "aa", "aux", "aux+aa")
SCENES = tuple(IC.B_RAW_SCENES)                    # M1, M4, M9, M16, deg1-M16, colors, P257-M9
S_SCENES = ("M1", "M4", "M9")                      # plain, _vec and _staged form of the absgrad kernels
E_SCENES = ("M1", "M16", "M9")                     # plain, _vec and _staged form, edge activations
V_SCENE = CR.INSTANCE_SCENE

# ---- the constants of the bars, each four times what the float32 twins of tests/_raw_ref.py need (same rounding
# points, another order).  tests/test_raw_cases_host.py measures the shares again and holds these to them; none comes from a GPU.
TWIN_SHARE = 0.66                                # largest (|twin - ref2| - 1e-5) / (2^-24 bud2), tables R and E, all twins
KAPPA_RAW = max(KAPPA, 4 * TWIN_SHARE)             # |gpu - ref2| <= 1e-5 + KAPPA_RAW 2^-24 bud2
TWIN_CONIC_UNITS, TWIN_OPACITY_UNITS = 49.0, 7.0  # twins' largest forward deviation, 2^-24 of the row's largest conic entry / opacity
CONIC_UNITS, OPACITY_UNITS = 4 * TWIN_CONIC_UNITS, 4 * TWIN_OPACITY_UNITS
TWIN_SHARE_V = 4.2                               # the same for the camera's 35 values over table V (beyond 1e-5 + carried)
K_RAW = int(math.ceil(4 * TWIN_SHARE_V))           # |gpu - ref| <= 1e-5 + carried + K_RAW 2^-24 budget
PERTURB_SEEDS = (1, 2)                             # the two +-2 ulp twins

# Row norms exp(1.5 N(0, 1)), one seed per scene: 900 + the scene's position.  A seed stands if the oracle alone keeps every case
# of the scene within `caps` (tests/test_raw_cases_host.py asserts that; the first seeds tried all do), else the next one up is
# taken -- judged on the oracle, never on a GPU outcome.
NORM_SEED = {"M1": 900, "M4": 901, "M9": 902, "M16": 903, "deg1-M16": 904, "colors": 905, "P257-M9": 906, V_SCENE: 907}


def _case(table, scene, feature, **kw):
    tag = {"R": "", "S": "abs-", "E": "edge-", "V": "camera-"}[table]
    return dict(id=f"{tag}{scene}-{feature}", table=table, scene=None if table == "V" else scene, feature=feature,
                edge=table == "E", absgrad=table == "S", options=dict(IC.DEFAULTS), raw=True, **kw)


TABLE_R = [_case("R", s, f) for s in SCENES for f in FEATURES]
TABLE_S = [_case("S", s, f) for s in S_SCENES for f in FEATURES]
TABLE_E = [_case("E", s, f) for s in E_SCENES for f in FEATURES]
TABLE_V = [_case("V", V_SCENE, f) for f in FEATURES]
ALL = TABLE_R + TABLE_S + TABLE_E + TABLE_V


def has_aa(case):
    return "aa" in case["feature"]


def has_aux(case):
    return "aux" in case["feature"]


def scene_name(case):
    return V_SCENE if case["table"] == "V" else case["scene"]


def activated_scene(case):
    """the scene's activated inputs as tests/_instance_cases.py / tests/_camera_grad_ref.py build them (cached: do not modify)"""
    return _activated_scene(scene_name(case), case["table"] == "V")


@functools.lru_cache(maxsize=None)
def _activated_scene(name, camera):
    return CR.SCENES[name]() if camera else IC.inputs(dict(scene=name))


def norms(name, P):
    return np.exp(1.5 * np.random.RandomState(NORM_SEED[name]).randn(P)).astype(np.float32)


# ---- table E: the rows set by hand.  (quaternion norm or None, quaternion or None, log-scales or None, logit or None)
UNDER = (3e-13, 4e-13, 0.0, 0.0)                   # norm 5e-13, under the clamp
EDGE_ROWS = (
    (3.4, None, None, None), (0.01, None, None, None), (1e-6, None, None, None), (1e6, None, None, None),
    (None, (0.0, 0.0, 0.0, 0.0), None, None),      # the zero quaternion
    (None, UNDER, None, None),
    (None, None, (-9.0, -9.0, -9.0), 3.0),         # only the 0.3 low-pass remains (h at its floor: o h = 1.21 / 255)
    (None, None, (None, -2.5, None), None),        # one long axis
    (None, None, None, -10.0),                     # under 1 / 255: in no pixel
    (None, None, None, -5.0), (None, None, None, 10.0),
    (None, None, None, 17.0),                      # sg rounds to 1: a float32 derivative of exactly 0
    (None, (0.0, 0.0, 0.0, 0.0), (-2.5, None, None), 10.0),
    (None, (0.0, 0.0, -5e-13, 0.0), None, -5.0),
    (1e6, None, (-9.0, -9.0, -9.0), -1.0),         # (with anti-aliasing o h = 0.34 / 255: in no pixel)
    (1e-6, None, None, 17.0),
)
UNDER_FLOOR_ROWS = (8,)                            # rows whose opacity is under 1 / 255: every gradient exactly 0
UNDER_CLAMP_ROWS = (5, 13)
ZERO_QUATERNION_ROWS = (4, 12)


def edge_rows(case):
    """the indices of the Gaussians set by hand: the first len(EDGE_ROWS) whose centre the scene's own oracle forward puts at
    least two pixels inside the image (a row shrunk to the 0.3 low-pass still touches a tile there)"""
    o = IC.reference(dict(scene=case["scene"], feature="aux"))["o"]
    x, y = o["xy"][:, 0], o["xy"][:, 1]
    inside = (o["radii"] > 0) & (x >= 2) & (x <= o["W"] - 3) & (y >= 2) & (y <= o["H"] - 3)
    return np.nonzero(inside)[0][:len(EDGE_ROWS)]


def raw_inputs(case):
    """the raw inputs of a case (cached: do not modify)"""
    return _raw_inputs(scene_name(case), case["table"] == "V", case["edge"])


@functools.lru_cache(maxsize=None)
def _raw_inputs(name, camera, edge):
    d = _activated_scene(name, camera)
    raw = RR.raw_inputs(d, norms(name, d["P"]))
    if not edge:
        return raw
    rot, sc, op = raw["rotations"].clone(), raw["scales"].clone(), raw["opacities"].clone()
    for i, (qn, q, ls, logit) in zip(edge_rows(dict(scene=name)), EDGE_ROWS):
        if qn is not None:
            rot[i] = d["rotations"][i] * np.float32(qn)
        if q is not None:
            rot[i] = torch.tensor(q, dtype=torch.float32)
        for k, v in enumerate(ls or ()):
            if v is not None:
                sc[i, k] = v
        if logit is not None:
            op.view(-1)[i] = logit
    return dict(raw, rotations=rot.contiguous(), scales=sc.contiguous(), opacities=op.contiguous())


def reference(case):
    """dict(raw, act, o, frag, cond): the raw inputs, their float64 activations rounded once (tests/_raw_ref.py::activated64), the
    oracle forward on them (at float32(o_eff) with anti-aliasing), its fragile pixels at IC.RAW_WINDOW and the largest conditioning
    of h over the visible Gaussians (0 without anti-aliasing).  Cached: do not modify."""
    return _reference(scene_name(case), case["table"] == "V", case["edge"], has_aa(case))


@functools.lru_cache(maxsize=None)
def _reference(name, camera, edge, aa):
    from oracle import ggd_oracle as O
    raw = _raw_inputs(name, camera, edge)
    act = RR.activated64(raw)
    o = run_oracle(RR.oracle_inputs(act, aa))
    cond = 0.0
    if aa:
        cond = float(AA.h_and_conditioning(act)[1][o["radii"] > 0].max(initial=0.0))
    return dict(raw=raw, act=act, o=o, frag=O.fragile_pixels(o, window=IC.RAW_WINDOW), cond=cond)


def caps(case):
    """(fragile pixels, fragile Gaussians) the reference alone may show: half of the helpers' caps (fragile_pixels: 2 + W H //
    5000; check_gradients: max(4, P // 1000)), so that a GPU run has the other half as its margin.  A camera case may leave no
    Gaussian out of its sums: 0."""
    d = activated_scene(case)
    return (2 + d["W"] * d["H"] // 5000) // 2, 0 if case["table"] == "V" else max(4, d["P"] // 1000) // 2


# ---- the launchers' dispatch rules for a raw case, restated (csrc/ggd_preprocess.hip::ggd_launch_preprocess,
# csrc/ggd_preprocess_bwd.hip::ggd_launch_preprocess_backward and its absgrad twin, csrc/ggd_camera.hip, csrc/ggd_normals.hip)
def _layout(d):
    M = 0 if d["shs"] is None else int(d["shs"].shape[1])
    staged = d["colors_precomp"] is None and M > 1
    return staged, staged and M <= 16 and (3 * M) % 4 == 0


def _b(v):
    return "true" if v else "false"


def preprocess_instances(case):
    """the forward per-Gaussian kernels of a case's two frames (the first is never folded, the second is under the defaults)"""
    _, shvec = _layout(activated_scene(case))
    folded = case["options"]["fold"] != 0 and case["options"]["binning"] != 0
    frames = {False} if case["table"] == "V" else {False, folded}     # (a camera case renders one frame)
    return {f"preprocess_kernel<{_b(shvec)}, {_b(fo)}, {_b(has_aa(case))}>" for fo in frames}


def preprocess_backward_instance(case):
    staged, shvec = _layout(activated_scene(case))
    stem = "preprocess_abs_backward" if case["absgrad"] else "preprocess_backward"
    aa, aux = _b(has_aa(case)), _b(has_aux(case))
    if shvec:
        return f"{stem}_vec_kernel<{aa}, {aux}>"
    if staged:
        return f"{stem}_staged_kernel<false, {aa}, {aux}>"
    return f"{stem}_kernel<{aa}, {aux}>"


def camera_instance(case):
    return f"camera_partial_kernel<{_b(has_aa(case))}, {_b(has_aux(case))}>" if case["table"] == "V" else None


def instances(case):
    """every kernel with a raw branch that a case runs"""
    out = set(preprocess_instances(case)) | {preprocess_backward_instance(case)}
    if case["table"] == "V":
        out.add(camera_instance(case))
    return out


NORMALS_INSTANCES = {"gaussian_normals_kernel", "gaussian_normals_backward_kernel"}


def every_instance():
    """the kernels the issue names: 24 per-Gaussian backward kernels, the four camera kernels, the forward kernel's SHVEC x FOLD x AA
    (a folded frame needs a tile-binning path, which the defaults take), and the two normals kernels"""
    tf = ("false", "true")
    out = set()
    for stem in ("preprocess_backward", "preprocess_abs_backward"):
        for aa in tf:
            for aux in tf:
                out |= {f"{stem}_kernel<{aa}, {aux}>", f"{stem}_vec_kernel<{aa}, {aux}>", f"{stem}_staged_kernel<false, {aa}, {aux}>"}
    out |= {f"camera_partial_kernel<{aa}, {aux}>" for aa in tf for aux in tf}
    out |= {f"preprocess_kernel<{sv}, {fo}, {aa}>" for sv in tf for fo in tf for aa in tf}
    return out | NORMALS_INSTANCES
