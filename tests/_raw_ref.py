"""Reference, budgets and float32 twin of the raw-attribute path (`raw_attributes`: the kernels take log-scales, unnormalised
quaternions and logits and apply exp / normalize / sigmoid themselves, with the three Jacobians in the per-Gaussian backward).
CPU only; DESIGN.md section 6zh.

The reference: the activations in float64, rounded once to float32 (`activated64`); the oracle's forward on those inputs (at
float32(o_eff) for an anti-aliasing case, as tests/_instance_cases.py::_reference); the float64 gradients and budgets with respect to
the ACTIVATED attributes from the project's references (`activated_reference`); the three Jacobians in float64 with the budgets taken
through them (`chain`).  The twin (`twin32`): the same pipeline in numpy float32 -- float32 activations, oracle.forward,
oracle.backward, float32 Jacobians in the kernel's order of operations -- optionally with every activated scale, quaternion entry
and opacity moved by +-2 ulp (a device expf / divide that is not correctly rounded).  Nothing here is taken from a kernel's result."""
from __future__ import annotations

import numpy as np
import torch

import _absgrad_ref as AG
import _antialias_ref as AA
import _camera_grad_ref as CR
import _depth_alpha_ref as DA
from _util import ATOL, EPS32, KAPPA, backward_reference, run_oracle

CLAMP = 1e-12     # torch.nn.functional.normalize's eps, the kernels' 1e-12f


def raw_inputs(d, norms):
    """d before its activations: log-scales and logits stored in float32 (as tests/_instance_cases.py::raw_inputs), the unit
    quaternions multiplied row-wise by `norms` [P]"""
    n = torch.as_tensor(np.asarray(norms, np.float32)).reshape(-1, 1)
    return dict(d, opacities=torch.logit(d["opacities"].double()).float().contiguous(),
                scales=torch.log(d["scales"]).contiguous(), rotations=(d["rotations"] * n).contiguous())


def activate(raw, dtype):
    """(s [P,3], q_hat [P,4], o [P], ||q|| [P,1]) in `dtype`, in the kernels' order of operations (ggd_math.h::act_normalize,
    act_sigmoid; expf)"""
    dt = np.dtype(dtype).type
    ls, q, x = (raw[k].numpy().astype(dtype) for k in ("scales", "rotations", "opacities"))
    with np.errstate(over="ignore"):
        s = np.exp(ls)
        norm = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + (q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]))[:, None]
        qh = q / np.maximum(norm, dt(CLAMP))
        o = dt(1) / (dt(1) + np.exp(-x.reshape(-1)))
    return s, qh, o, norm


def _as_inputs(raw, s, qh, o):
    f = lambda a, like: torch.from_numpy(np.ascontiguousarray(a, np.float32)).reshape(like.shape).contiguous()
    return dict(raw, scales=f(s, raw["scales"]), rotations=f(qh, raw["rotations"]), opacities=f(o, raw["opacities"]))


def activated64(raw):
    """the activated inputs: exp, x / max(||x||, 1e-12) and sigmoid in float64, rounded once to float32"""
    return _as_inputs(raw, *activate(raw, np.float64)[:3])


def activated32(raw, perturb_seed=None):
    """the twin's activated inputs: the same in numpy float32; with a seed, every non-zero entry of the three arrays moved by two
    ulps up or down (seeded signs), the opacities kept within [0, 1]"""
    s, qh, o, _ = activate(raw, np.float32)
    if perturb_seed is not None:
        rng = np.random.RandomState(perturb_seed)

        def move(a):
            step = (2 * (2 * rng.randint(0, 2, size=a.shape) - 1)).astype(np.int32)
            bits = a.view(np.int32) + np.where(a != 0, step, 0).astype(np.int32)
            return bits.view(np.float32)
        s, qh, o = move(s), move(qh), np.minimum(move(o), np.float32(1))
    return _as_inputs(raw, s, qh, o)


def oracle_inputs(act, aa):
    """what the oracle blends: the activated inputs, for an anti-aliasing case with the opacities replaced by float32(o h)"""
    if not aa:
        return act
    oe = torch.from_numpy(AA.o_eff(act).astype(np.float32)).reshape(act["opacities"].shape).contiguous()
    return dict(act, opacities=oe)


def backward_state(o, n=None):
    """what the reference backward reads of a forward: the per-Gaussian records of the oracle forward `o` (the native run's are
    held to them by the forward check, not bit for bit) with the per-pixel state and the lists of the native forward `n`, which
    its backward consumes (default: the oracle's own)"""
    src = o if n is None else n
    return dict(radii=torch.from_numpy(np.asarray(o["radii"])), xy=o["xy"], conic_opacity=o["conic_opacity"], rgb=o["rgb"],
                final_T=src["final_T"], n_contrib=src["n_contrib"], point_list=src["point_list"], ranges=src["ranges"],
                num_rendered=src["num_rendered"])


def activated_reference(act, o, feature, g, gD, gA, n=None, absgrad=False, kappa=KAPPA):
    """dict(blend=(ref, bud), ref, bud, frag): float64 gradients and budgets with respect to the activated attributes of `act` for
    the oracle forward `o` of oracle_inputs(act, aa).  `blend`: the sums before the anti-aliasing chain (what the camera's reference
    starts from); ref / bud: after it.  backward_ref64 for a plain case, tests/_depth_alpha_ref.py for the depth / alpha maps,
    tests/_absgrad_ref.py for absgrad, tests/_antialias_ref.py::compose_backward for anti-aliasing (its allowance for the h chain's own
    arithmetic is stated absolutely: divided by the `kappa` check_gradients will multiply with)."""
    aa, aux = "aa" in feature, "aux" in feature
    d_o = oracle_inputs(act, aa)
    st = backward_state(o, n)
    g, gD, gA = (np.asarray(t, np.float32) for t in (g, gD, gA))
    if absgrad:
        ref, bud, frag, _ = AG.reference(d_o, o, st, g, gD if aux else None, gA if aux else None)
    elif aux:
        ref, bud, frag = DA.backward_ref(d_o, o, st, g, gD.reshape(o["H"], o["W"]), gA.reshape(o["H"], o["W"]))
    else:
        ref, bud, frag = backward_reference(d_o, o, st, g)
    blend = (ref, bud)
    if aa:
        ref, bud = AA.compose_backward(act, ref, bud, kappa=kappa)
    return dict(blend=blend, ref=ref, bud=bud, frag=frag)


def jacobians(acts, g_s, g_q, g_o):
    """J^T g of the three activations in the dtype of `acts` = (s, q_hat, o, ||q||), as the kernels write them
    (ggd_preprocess_bwd.hip: dscale *= s; ggd_math.h::act_normalize_backward; g (sg (1 - sg))).  Under the clamp q_hat = q / eps
    has the Jacobian I / eps: no projection term."""
    s, qh, o, norm = acts
    dt = s.dtype.type
    g_s, g_q, g_o = np.asarray(g_s).astype(s.dtype), np.asarray(g_q).astype(s.dtype), np.asarray(g_o).astype(s.dtype).reshape(-1)
    with np.errstate(over="ignore", invalid="ignore"):
        dot = ((qh[:, 0] * g_q[:, 0] + qh[:, 1] * g_q[:, 1]) + (qh[:, 2] * g_q[:, 2] + qh[:, 3] * g_q[:, 3]))[:, None]
        dn = np.maximum(norm, dt(CLAMP))
        gq = np.where(norm < dt(CLAMP), g_q / dn, (g_q - qh * dot) / dn)
        return g_s * s, gq, g_o * (o * (dt(1) - o))


def chain(raw, ref, bud):
    """(ref2, bud2): the gradients with respect to the activated attributes taken to the raw ones in float64, with the budgets
    (units of 2^-24, as check_gradients reads them) beside them.  The arrays no activation enters pass through unchanged."""
    s, qh, o, norm = acts = activate(raw, np.float64)
    gs, gq, go = jacobians(acts, ref["dL_dscales"], ref["dL_drots"], ref["dL_dopacity"])
    ref2, bud2 = dict(ref), dict(bud)
    shape_o = np.asarray(ref["dL_dopacity"]).shape
    ref2.update(dL_dscales=gs, dL_drots=gq, dL_dopacity=go.reshape(shape_o))
    # exp: dscale * s3.  The activated budget through |J| = s; three roundings relative to the result -- s3 itself (expf), the
    # product, and one of the factor mod s the result was built from (the existing test's term)
    bud2["dL_dscales"] = bud["dL_dscales"] * s + 3.0 * np.abs(gs)
    # normalize: (dq - q_hat (q_hat . dq)) / max(||q||, eps), or dq / eps under the clamp.  The activated budget and, eight
    # roundings deep (four products and three sums of the dot, the product with q_hat, the difference, the divide: the existing
    # test's term), |dq| itself go through |J| = (I + |q_hat| |q_hat|^T) / max(||q||, eps) -- I / eps under the clamp
    under = norm < CLAMP
    dn = np.maximum(norm, CLAMP)
    aq = np.abs(qh)
    absj = lambda v: np.where(under, v, v + aq * (aq * v).sum(1, keepdims=True)) / dn
    # + ||q|| = sqrtf((x x + y y) + (z z + w w)) is itself rounded: squares and two sums (halved by the root) and the root, below
    #   three roundings relative to the divisor and so to the result; the constant 1e-12f is within half an ulp of 1e-12
    bud2["dL_drots"] = absj(bud["dL_drots"]) + 8.0 * absj(np.abs(ref["dL_drots"])) + 3.0 * np.abs(gq)
    # sigmoid: g_op * (sg * (1 - sg)).  The activated budget through |J| = o (1 - o); four roundings relative to the result (1 - sg,
    # the two products, and one of g_op's own scaling: the existing test's term)
    g_o, b_o = np.abs(np.asarray(ref["dL_dopacity"], np.float64)).reshape(-1), np.asarray(bud["dL_dopacity"], np.float64).reshape(-1)
    # + sg = 1 / (1 + expf(-x)) carries four roundings of its own (expf within an ulp = 2, the sum, the divide): 4 2^-24 sg,
    #   absolute.  1 - sg is formed from that rounded sg, so the error enters sg (1 - sg) through d/dsg = 1 - 2 sg, NOT relative to
    #   1 - sg: at a logit of +10, 1 - sg = 4.5e-5 and half an ulp of sg is 6.6e-4 of it.  |dL/do| times 4 sg |1 - 2 sg|
    bud2["dL_dopacity"] = (b_o * o * (1.0 - o) + 4.0 * np.abs(go) + 4.0 * o * np.abs(1.0 - 2.0 * o) * g_o).reshape(shape_o)
    return ref2, bud2


def reference(raw, act, o, feature, g, gD, gA, n=None, absgrad=False, kappa=KAPPA):
    """dict(ref2, bud2, frag, blend): activated_reference pushed through `chain`"""
    r = activated_reference(act, o, feature, g, gD, gA, n=n, absgrad=absgrad, kappa=kappa)
    ref2, bud2 = chain(raw, r["ref"], r["bud"])
    return dict(ref2=ref2, bud2=bud2, frag=r["frag"], blend=r["blend"])


def twin32(raw, feature, g, gD, gA, perturb_seed=None):
    """dict(o, act, grads): the float32 twin.  act / o: the float32-activated inputs (perturbed with a seed) and the float32 oracle
    forward on them; grads: oracle.backward's arrays taken through the float32 Jacobians (the depth / alpha maps through the
    pseudo-colour of tests/_depth_alpha_ref.py, the anti-aliasing h chain from tests/_antialias_ref.py::vjp on the twin's inputs --
    that helper has no float32 form -- added in float32)."""
    from oracle import ggd_oracle as O
    aa, aux = "aa" in feature, "aux" in feature
    f32 = np.float32
    act = activated32(raw, perturb_seed)
    o = run_oracle(oracle_inputs(act, aa))
    b = O.backward(o, np.asarray(g, f32))
    if aux:
        rgb = DA.pseudo_rgb(o)
        g_aux = np.stack([np.asarray(gD, f32).reshape(o["H"], o["W"]), np.asarray(gA, f32).reshape(o["H"], o["W"]),
                          np.zeros((o["H"], o["W"]), f32)])
        ba = O.backward(dict(o, rgb=rgb, bg=np.zeros(3, f32), colors_precomp=rgb), g_aux)
        for k in ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drots"):
            b[k] = b[k] + ba[k]
        vis = (o["radii"] > 0)
        gz = (ba["dL_dcolors"][:, 0] * vis).astype(f32)
        v = np.asarray(o["viewmatrix"], f32).reshape(-1)
        b["dL_dmeans3D"] = b["dL_dmeans3D"] + gz[:, None] * np.array([v[2], v[6], v[10]], f32)[None, :]
    if aa:
        h = AA.vjp(act, b["dL_dopacity"].astype(np.float64))
        b["dL_dopacity"] = h["dL_dopacity"].reshape(-1).astype(f32)
        for k in ("dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drots"):
            b[k] = b[k] + h[k].reshape(b[k].shape).astype(f32)
    acts = (act["scales"].numpy(), act["rotations"].numpy(), act["opacities"].numpy().reshape(-1), activate(raw, f32)[3])
    gs, gq, go = jacobians(acts, b["dL_dscales"], b["dL_drots"], b["dL_dopacity"])
    grads = dict(b, dL_dscales=gs, dL_drots=gq, dL_dopacity=go)
    grads.pop("dL_dconic")
    return dict(o=o, act=act, grads=grads)


def share(got, ref2, bud2, frag):
    """per array, the factor on 2^-24 bud2 that `got` needs beyond the 1e-5 floor: max (|got - ref2| - 1e-5) / (2^-24 bud2) over
    the rows that are not fragile; an element without a budget must be met within the floor"""
    out = {}
    keep = ~(np.asarray(frag) > 0)
    for k, r in ref2.items():
        if r is None or k == "dL_dconic" or got.get(k) is None:
            continue
        over = np.maximum(np.abs(np.asarray(got[k], np.float64).reshape(r.shape) - r) - ATOL, 0.0)[keep]
        b = np.asarray(bud2[k], np.float64).reshape(r.shape)[keep]
        assert (over[b == 0] == 0).all(), k
        out[k] = float((over[b > 0] / (EPS32 * b[b > 0])).max(initial=0.0))
    return out


def forward_deviation(o, t):
    """(conic, opacity): the largest deviation of the twin forward `t` from the reference forward `o` over the visible rows, in
    units of 2^-24 of the row's largest conic entry and of the opacity"""
    vis = o["radii"] > 0
    c, ct = o["conic_opacity"][vis].astype(np.float64), t["conic_opacity"][vis].astype(np.float64)
    dev_c = np.abs(ct[:, :3] - c[:, :3]).max(1) / (EPS32 * np.abs(c[:, :3]).max(1))
    dev_o = np.abs(ct[:, 3] - c[:, 3]) / (EPS32 * np.maximum(np.abs(c[:, 3]), 1e-300))
    return float(dev_c.max(initial=0.0)), float(dev_o.max(initial=0.0))


def camera_reference(act, o, feature, blend, gD, gA, n=None):
    """dict(val [35], bud [35], car [35], gz, gzb) of the camera's gradients: tests/_camera_grad_ref.py::reference on the
    float64-activated oracle `o` and the blend sums of activated_reference (before the anti-aliasing chain, which `terms` restates
    from the activated opacities)"""
    aa, aux = "aa" in feature, "aux" in feature
    gz = gzb = None
    if aux:
        lists = None if n is None else backward_state(o, n)
        gz, gzb = CR.depth_slot(o, np.asarray(gD, np.float32).reshape(o["H"], o["W"]),
                                np.asarray(gA, np.float32).reshape(o["H"], o["W"]), lists)
    ref, bud = blend
    op = act["opacities"].numpy().reshape(-1) if aa else None
    val, b, car, _ = CR.reference(o, ref, bud, gz, gzb, aa_opacity=op)
    return dict(val=val, bud=b, car=car, gz=gz, gzb=gzb, aa_opacity=op)


def camera_share(cam, o, blend, twin_forward, twin_act):
    """tests/_camera_grad_ref.py::share with the twin's terms evaluated on the TWIN's forward (its covariance and opacities come from
    the float32 activations, as camera_partial_kernel recomputes them with raw = 1) and the reference's sums: the largest
    |twin - ref64| / (2^-24 budget) over the 35 values beyond the float32 rounding of the sums themselves"""
    ref = blend[0]
    aa_t = None if cam["aa_opacity"] is None else twin_act["opacities"].numpy().reshape(-1)
    tw = CR.twin32(twin_forward, ref, cam["gz"], aa_t)
    a = CR._slots(ref, cam["gz"], o["P"])
    rounding = np.zeros(35)
    for j in range(CR.NSLOT):
        one = np.zeros_like(a); one[:, j] = np.abs(a[:, j] - a[:, j].astype(np.float32).astype(np.float64))
        t, _ = CR.terms(o, *CR._split(one), dtype=np.float64, aa_opacity=cam["aa_opacity"])
        rounding += np.abs(t).sum(0)
    err = np.maximum(np.abs(tw - cam["val"]) - rounding, 0.0)
    bud = cam["bud"]
    return float((err / np.maximum(EPS32 * bud, 1e-300))[bud > 0].max(initial=0.0))
