"""The C ABI's own argument checking (ggd_capi.hip), called straight through ctypes: the Python wrapper refuses most bad input
before the library sees it, so nothing else pins what the entry points themselves return.  Every row is (entry point, what is
wrong, return code, substring of ggd_last_error); each returns from validation before anything is enqueued, so the file
launches nothing but the two small frames of the last test.

The scene is P = 4 Gaussians on a 16 x 16 image with M = 1 SH coefficient; every pointer that is not the one under test is a
small real device tensor of the right size.  One context (of a stream of its own, so that the option and speculation state of
the other tests' context is not touched) serves the whole table and, afterwards, an ordinary render: a refused call leaves the
context usable."""
import ctypes as C
import os
import re

import pytest
import torch

from _util import scene_inputs, device_args, same_frame

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

P, W, H, M = 4, 16, 16, 1
CAP = 64          # instances the binning buffer is laid out for

INPUTS = ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")
GRADS = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drots")
BWD_HEAD = INPUTS + ("radii", "geom_buf", "binning_buf", "img_buf", "R", "dL_dpix")
ORDER = {
    "ggd_forward_geometry": INPUTS + ("geom_buf", "radii", "num_rendered"),
    "ggd_forward_render": ("geom_buf", "R", "binning_buf", "img_buf", "out_color"),
    "ggd_forward_render_aux": ("geom_buf", "R", "binning_buf", "img_buf", "out_color", "out_depth", "out_alpha"),
    "ggd_forward": INPUTS + ("geom_buf", "radii", "binning_buf", "capacity", "img_buf", "out_color", "num_rendered"),
    "ggd_forward_aux": INPUTS + ("geom_buf", "radii", "binning_buf", "capacity", "img_buf", "out_color", "out_depth", "out_alpha",
                                 "num_rendered"),
    "ggd_forward_enqueue": INPUTS + ("geom_buf", "radii", "binning_buf", "capacity", "img_buf", "out_color"),
    "ggd_backward": BWD_HEAD + GRADS,
    "ggd_backward_aux": BWD_HEAD + ("dL_ddepth", "dL_dalpha") + GRADS,
    "ggd_backward_abs": BWD_HEAD + ("dL_ddepth", "dL_dalpha") + GRADS + ("dL_dmeans2D_abs",),
}
BACKWARDS = ("ggd_backward", "ggd_backward_aux", "ggd_backward_abs")
# the default call: SHs (no precomputed colours), scales + rotations (no precomputed covariance)
ABSENT = {"colors_precomp": None, "cov3D_precomp": None}
COV = {"scales": None, "rotations": None, "cov3D_precomp": "cov3D_precomp"}   # value: the tensor passed in that slot
ALL_NULL = {n: None for names in ORDER.values() for n in names if n not in ("R", "capacity", "num_rendered")}

# (entry point, ggd_params fields changed -- None: prm itself is NULL, arguments changed, return code, message)
GEOMETRY = [
    (None, {}, -1, "params is NULL"),
    ({"width": 0}, {}, -1, "bad P / image size"),
    ({"viewmatrix": None}, {}, -1, "must be device pointers"),
    ({"sh_degree": 4}, {}, -1, "sh_degree must be 0..3"),
    ({"tanfovx": 0.0}, {}, -1, "tanfov must be non-zero"),
    ({}, {"means3D": None}, -1, "means3D is NULL"),
    ({}, {"colors_precomp": "colors_precomp"}, -1, "one of either SHs or precomputed colors"),
    ({}, {"shs": None}, -1, "one of either SHs or precomputed colors"),
    ({}, {"rotations": None}, -1, "scale/rotation pair or precomputed 3D covariance"),
    ({}, {"cov3D_precomp": "cov3D_precomp"}, -1, "scale/rotation pair or precomputed 3D covariance"),
    ({}, {"scales": None, "rotations": None}, -1, "scale/rotation pair or precomputed 3D covariance"),
    ({"sh_degree": 1}, {}, -1, "fewer coefficients"),
    ({}, {"num_rendered": None}, -1, "num_rendered is NULL"),
    ({}, {"geom_buf": None}, -1, "geom_buf / radii / opacities is NULL"),
    ({}, {"radii": None}, -1, "geom_buf / radii / opacities is NULL"),
    ({}, {"opacities": None}, -1, "geom_buf / radii / opacities is NULL"),
    ({"raw_attributes": 1}, COV, -1, "raw_attributes needs scales/rotations"),
    # precedence of two simultaneous errors
    ({"width": 0}, {"means3D": None}, -1, "bad P / image size"),
    ({}, {"means3D": None, "num_rendered": None}, -1, "means3D is NULL"),
]
RENDER = [
    ({"R": -1}, "num_rendered < 0"),
    ({"img_buf": None}, "img_buf / out_color is NULL"),
    ({"out_color": None}, "img_buf / out_color is NULL"),
    ({"R": 5, "binning_buf": None}, "geom_buf / binning_buf is NULL"),
]
ROWS = [("ggd_forward_geometry",) + r for r in GEOMETRY]
ROWS += [(fn, {}, over, -1, msg) for fn in ("ggd_forward_render", "ggd_forward_render_aux") for over, msg in RENDER]
ROWS += [
    ("ggd_forward_render_aux", {}, {"out_alpha": None}, -1, "out_depth / out_alpha is NULL"),
    ("ggd_forward", {}, {"capacity": -1}, -1, "capacity < 0"),
    ("ggd_forward_aux", {}, {"out_depth": None}, -1, "out_depth / out_alpha is NULL"),
    ("ggd_forward_enqueue", {}, {"capacity": 0}, -1, "needs the tile-binning path"),
]
for _fn in BACKWARDS:
    # radii, geom_buf, img_buf, dL_dpix, the seven gradient arrays every mode needs and (M = 1 > 0) dL_dsh, each NULL in turn
    ROWS += [(_fn, {}, {n: None}, -1, "ggd_backward: NULL buffer") for n in ("radii", "geom_buf", "img_buf", "dL_dpix") + GRADS]
    ROWS += [
        (_fn, {}, {"R": 5, "binning_buf": None}, -1, "NULL buffer"),
        (_fn, {"raw_attributes": 1}, {"opacities": None}, -1, "raw_attributes needs opacities"),
        (_fn, {"antialiasing": 1}, {"opacities": None}, -1, "antialiasing needs the opacities"),
        (_fn, {"P": 0}, ALL_NULL, 0, ""),
    ]
ROWS.append(("ggd_backward_abs", {}, {"dL_dmeans2D_abs": None}, -1, "NULL dL_dmeans2D_abs"))
# P = 0: every input and buffer pointer NULL is a valid (empty) frame; *num_rendered is set to 0
ROWS.append(("ggd_forward_geometry", {"P": 0}, ALL_NULL, 0, ""))


class _Env:
    def __init__(self):
        from gaussian_gan_decoder_amd import _capi
        self.capi = _capi
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.Stream(device=self.dev)
        with torch.cuda.stream(self.stream):
            self.ctx, self.handle = _capi.context_and_stream(self.dev)
        self.lib = lib = self.ctx.lib
        d = scene_inputs(P=P, size=W)
        assert d["shs"].shape == (P, M, 3)
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.dev)
        u8 = lambda n: torch.zeros((int(n),), dtype=torch.uint8, device=self.dev)
        self.t = {k: d[k].to(self.dev).contiguous() for k in ("means3D", "shs", "opacities", "scales", "rotations", "viewmatrix",
                                                              "projmatrix", "campos", "bg")}
        self.t.update(colors_precomp=f32(P, 3) + 0.5, cov3D_precomp=f32(P, 6), radii=torch.zeros(P, dtype=torch.int32, device=self.dev),
                      geom_buf=u8(lib.ggd_geom_bytes(P)), binning_buf=u8(lib.ggd_binning_bytes(CAP)), img_buf=u8(lib.ggd_img_bytes(W, H)),
                      out_color=f32(3, H, W), out_depth=f32(1, H, W), out_alpha=f32(1, H, W), dL_dpix=f32(3, H, W),
                      dL_ddepth=f32(1, H, W), dL_dalpha=f32(1, H, W), dL_dmeans2D=f32(P, 3), dL_dcolors=f32(P, 3),
                      dL_dopacity=f32(P, 1), dL_dmeans3D=f32(P, 3), dL_dcov3D=f32(P, 6), dL_dsh=f32(P, M, 3), dL_dscales=f32(P, 3),
                      dL_drots=f32(P, 4), dL_dmeans2D_abs=f32(P, 3))
        self.prm = dict(P=P, M=M, sh_degree=0, width=W, height=H, tanfovx=d["tanfovx"], tanfovy=d["tanfovy"], scale_modifier=1.0,
                        prefiltered=0, debug=0, viewmatrix="viewmatrix", projmatrix="projmatrix", campos="campos", bg="bg",
                        raw_attributes=0, antialiasing=0)
        torch.cuda.synchronize(self.dev)
        self.scene8 = device_args(scene_inputs(P=8, size=16), device="cuda:0")

    def call(self, fn, prm_over, over):
        """One entry point with the default arguments except `over`; returns (return code, ggd_last_error, *num_rendered)."""
        prm = None
        if prm_over is not None:
            f = dict(self.prm, **prm_over)
            for k in ("viewmatrix", "projmatrix", "campos", "bg"):
                f[k] = None if f[k] is None else self.t[f[k]].data_ptr()
            prm = C.byref(self.capi.Params(**f))
        R = C.c_int64(77)
        default = {"R": 0, "capacity": CAP, **ABSENT}
        args = []
        for name in ORDER[fn]:
            v = over.get(name, default.get(name, name))      # an int, None (NULL) or the name of the tensor passed in that slot
            if name == "num_rendered":
                v = None if v is None else C.byref(R)
            elif isinstance(v, str):
                v = C.c_void_p(self.t[v].data_ptr())
            args.append(v)
        rc = getattr(self.lib, fn)(self.ctx.handle, C.c_void_p(self.handle), prm, *args)
        return rc, self.lib.ggd_last_error(self.ctx.handle).decode(), R.value

    def check_row(self, row):
        fn, prm_over, over, code, msg = row
        rc, err, R = self.call(fn, prm_over, over)
        assert rc == code, (row, rc, err)
        if code != 0:
            assert msg in err, (row, err)
        elif "num_rendered" in ORDER[fn]:
            assert R == 0, row

    def render8(self):
        from gaussian_gan_decoder_amd.rasterizer import rasterize_gaussians_native
        with torch.cuda.stream(self.stream):
            assert self.capi.context_and_stream(self.dev)[0] is self.ctx
            out = rasterize_gaussians_native(*self.scene8)
        torch.cuda.synchronize(self.dev)
        return out


@pytest.fixture(scope="module")
def env():
    return _Env()


def _row_id(row):
    fn, prm_over, over, code, msg = row
    what = ["prm=NULL"] if prm_over is None else [f"{k}={v}" for k, v in prm_over.items()]
    what += ["all NULL"] if over is ALL_NULL else [f"{k}={v}" for k, v in over.items()]
    return fn[4:] + ": " + ", ".join(what)


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_refusal(env, row):
    env.check_row(row)


def test_collect_without_a_pending_frame(env):
    R = C.c_int64(0)
    assert env.lib.ggd_forward_collect(env.ctx.handle, C.c_void_p(env.handle), C.byref(R)) == -1
    assert "no frame is pending" in env.lib.ggd_last_error(env.ctx.handle).decode()


def _options(env):
    """(GGD_OPT_COUNT, {option: its documented maximum}) -- include/ggd_raster.h"""
    c = env.capi
    hdr = open(os.path.join(ROOT, "include", "ggd_raster.h")).read()
    wgs_max = 1 << int(re.search(r"#define\s+GGD_PREPROCESS_WGS_MAX\s+\(1 << (\d+)\)", hdr).group(1))
    count = len(re.findall(r"^\s*GGD_OPT_[A-Z0-9_]+\s*=\s*\d+", hdr, flags=re.M))
    return count, {c.OPT_EXP_MODE: 3, c.OPT_BLEND_CULL: 1, c.OPT_BINNING: 3, c.OPT_BLEND_SPLIT: 4, c.OPT_FOLD: 1, c.OPT_MSD_SORT: 1,
                   c.OPT_PREPROCESS_WGS: wgs_max, c.OPT_L1_COUNTED: 1}


def test_option_values(env):
    lib, h, c = env.lib, env.ctx.handle, env.capi
    count, maxima = _options(env)
    assert count == len(maxima) == 8
    assert lib.ggd_set_option(h, c.OPT_BLEND_SPLIT, 5) == -1
    assert lib.ggd_set_option(h, count, 0) == -1            # GGD_OPT_COUNT is no option
    old = {o: lib.ggd_get_option(h, o) for o in maxima}
    try:
        for o, top in maxima.items():
            assert lib.ggd_set_option(h, o, top) == 0, o
            assert lib.ggd_get_option(h, o) == top, o
            assert lib.ggd_set_option(h, o, top + 1) == -1, o
            assert lib.ggd_get_option(h, o) == top, o
    finally:
        for o, v in old.items():
            assert lib.ggd_set_option(h, o, v) == 0
    assert {o: lib.ggd_get_option(h, o) for o in maxima} == old


def test_context_still_usable_after_the_whole_table(env):
    """An ordinary frame rendered on the table's context before and after every refusal above is the same frame."""
    before = env.render8()
    for row in ROWS:
        env.check_row(row)
    test_collect_without_a_pending_frame(env)
    test_option_values(env)
    after = env.render8()
    assert before[0] > 0
    assert same_frame(before, after)
