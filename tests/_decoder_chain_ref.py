"""TEST-ONLY restatement of the fused decoder for the three decoder chains (csrc/ggd_mlp.hip: THE THREE CHAINS; DESIGN.md
section 6r): tests/_decoder_ref.py::decoder_ref generalised by the chain table, with the same rounding hooks (the Tier objects,
the GELU polynomials and the seeded inputs are _decoder_ref's, imported, not copied).  For chain 0 it performs decoder_ref's
operations in decoder_ref's order and is bit-equal to it (tests/test_decoder_chains_host.py).  Never imported by the product.

The five ATTRIBUTES keep their public attrs columns in every chain (a: 0 colour, 1 opacity, 2 rotation, 3 scale, 4 xyz; columns
A0[a] .. A0[a] + OD[a]).  A chain is the order in which they are decoded and what each head sees:
  chain 0 sequential_reversed  order 0 1 2 3 4   n_extra 0 3 4 8 11    scale -softplus(s + 5) - 2.5
  chain 1 sequential           order 4 3 2 1 0   n_extra 0 3 6 10 11   scale -softplus(s + 5) - 2
  chain 2 parallel             order 4 3 2 1 0   n_extra 0 0 0 0 0     scale -softplus(s + 5) - 2
Everything per head (params, dout, grads) is indexed by EXECUTION POSITION h.
  forward, position h:  x0 = [feat(32) | pos(3) | attrs[:, cols[:n_extra[h]]]], cols = the public columns of the earlier
                        positions in execution order;  the MLP as in decoder_ref;  the activation of attribute order[h]
  backward, h = 4..0:   d = dattrs[:, columns of order[h]]  (+ dinfo[:, 3 + seen[h] ..] if a later position reads them: never
                        the last position, never in chain 2);  scale: * -sigmoid;  xyz: * 0.01 (so the first head of chain 1
                        receives 0.01 (dattrs + dinfo));  dinfo [N,16] is in the chain's SLOT order (slots 0..2 position,
                        3 + k the k-th chained input)
"""
from types import SimpleNamespace

import torch

import _decoder_ref as R
from _decoder_ref import IDENTITY, TIERS, make_inputs   # noqa: F401  (the tests take them from here)

A0, OD = R.A0, R.OD           # by attribute
ATTRS = R.HEADS               # module names by attribute


class Chain:
    def __init__(self, cid, name, order, chained, scale_c):
        self.id, self.name, self.order, self.chained, self.scale_c = cid, name, tuple(order), chained, scale_c
        self.heads = tuple(ATTRS[a] for a in self.order)
        self.od = tuple(OD[a] for a in self.order)
        self.seen = tuple(sum(self.od[:h]) for h in range(5))              # outputs decoded before position h
        self.n_extra = self.seen if chained else (0,) * 5
        self.in_features = tuple(35 + n for n in self.n_extra)
        self.cols = [A0[a] + e for a in self.order for e in range(OD[a])]  # info slot 3 + k -> public column (chained chains)

    def reads_back(self, h):
        return self.chained and h != 4


CHAINS = (Chain(0, "sequential_reversed", (0, 1, 2, 3, 4), True, 2.5),
          Chain(1, "sequential", (4, 3, 2, 1, 0), True, 2.0),
          Chain(2, "parallel", (4, 3, 2, 1, 0), False, 2.0))


def module_class(chain):
    from gaussian_gan_decoder_amd import decoder as D
    return (D.SequentialDecoderReverse, D.SequentialDecoder, D.ParallelDecoder)[CHAINS[chain].id]


def module_params(mod, chain, dtype=None, device=None):
    """The 40 tensors (W1 b1 .. W4 b4 per head) in the chain's execution order == the order of the module's own parameters()"""
    out = []
    for name in CHAINS[chain].heads:
        bb = getattr(mod, name).backbone
        for k in (0, 2, 4, 6):
            out += [bb[k].weight.detach(), bb[k].bias.detach()]
    return [p.to(dtype=dtype or p.dtype, device=device or p.device) for p in out]


def make_decoder(chain, seed=3):
    """_decoder_ref.make_decoder for the chain's module type: seeded, 2-D parameters * 1.5"""
    torch.manual_seed(seed)
    mod = module_class(chain)()
    for p in mod.parameters():
        if p.dim() == 2:
            p.data *= 1.5
    return mod


def only(dattrs, attr):
    """dattrs with every column but attribute `attr`'s zeroed (a loss on that attribute alone)"""
    d = torch.zeros_like(dattrs)
    d[:, A0[attr]:A0[attr] + OD[attr]] = dattrs[:, A0[attr]:A0[attr] + OD[attr]]
    return d


def decoder_chain_ref(chain, params, feats, pos, dattrs, tier=IDENTITY):
    """decoder_ref for chain `chain` (0, 1, 2): params in execution order -> attrs [N,16] (public columns), dfeat [N,32],
    dinfo [N,16] (slot order), dout [5,N,4] and grads (40), by execution position."""
    ch = CHAINS[chain]
    n = pos.shape[0]
    kw = dict(dtype=feats.dtype, device=feats.device)
    attrs = torch.zeros((n, 16), **kw)
    zs, x0s = [], []
    for h in range(5):
        a_ = ch.order[h]
        W = params[8 * h:8 * h + 8]
        x0 = torch.cat([feats, pos, attrs[:, ch.cols[:ch.n_extra[h]]]], 1)
        a, zh = x0, []
        for l in range(3):
            z = tier.fwd(a) @ tier.fwd(W[2 * l]).t() + W[2 * l + 1]
            zh.append(tier.z(z))
            a = tier.act(zh[-1] if tier.gelu_of_stored_z else z)
        raw = tier.fwd(a) @ tier.fwd(W[6]).t() + W[7]
        if a_ == 3:
            raw = -torch.nn.functional.softplus(raw + 5.0) - ch.scale_c
        elif a_ == 4:
            raw = raw * 0.01 + pos
        attrs[:, A0[a_]:A0[a_] + OD[a_]] = raw
        zs.append(zh)
        x0s.append(x0)

    dfeat = torch.zeros((n, 32), **kw)
    dinfo = torch.zeros((n, 16), **kw)
    dout = torch.zeros((5, n, 4), **kw)
    grads = [None] * 40
    ones = torch.ones((n, 1), **kw)
    for h in range(4, -1, -1):
        a_ = ch.order[h]
        W = params[8 * h:8 * h + 8]
        grad = tier.grad()
        d = dattrs[:, A0[a_]:A0[a_] + OD[a_]].clone()
        if ch.reads_back(h):
            d = d + dinfo[:, 3 + ch.seen[h]:3 + ch.seen[h] + OD[a_]]
        if a_ == 3:
            sp = -attrs[:, 8:11] - ch.scale_c
            d = d * -(1.0 - torch.exp(-sp))
        elif a_ == 4:
            d = d * 0.01
        dout[h, :, :OD[a_]] = d
        grad.begin_head(d)

        def wg(left, right, slot):
            L, Rt = grad.wgrad(left, torch.cat([right, ones], 1))
            g = L.t() @ Rt
            grads[8 * h + 2 * slot], grads[8 * h + 2 * slot + 1] = g[:, :-1], g[:, -1]

        wg(d, tier.act_wg(zs[h][2]), 3)
        dh = grad.operand(d) @ tier.wt(W[6])
        for l in (2, 1, 0):
            dz = dh * tier.dact(zs[h][l])
            wg(dz, tier.act_wg(zs[h][l - 1]) if l else x0s[h], l)
            dh = grad.operand(dz) @ tier.wt(W[2 * l])
        dfeat = dfeat + dh[:, :32]
        dinfo[:, :dh.shape[1] - 32] += dh[:, 32:]
    return SimpleNamespace(attrs=attrs, dfeat=dfeat, dinfo=dinfo, dout=dout, grads=grads)
