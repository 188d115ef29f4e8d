"""What the detectors' graph engines have in common, in one place (ssd300.SSD300 has an engine of its own):
  * the flat layout and the He-normal initialisation: `Row`, `param_layout`, `init_parameters`;
  * the dgrad-layout filter table: `filter_table`;
  * `SharedGradients` (YOLOv3, RetinaNet, FCOS): a residual sum and its operands share ONE gradient buffer, found through `gid` -- find / union,
    the reverse pass that decides who writes a buffer first and who accumulates, one buffer per written group, `grad_of`;
  * the pre-activation ResNet + pyramid of RetinaNet and FCOS: `new_act`, `conv_desc`, `preact_resnet`, `fpn`, `trunk_fwd`, `trunk_bwd`;
  * `OwnedGradients` (CenterNet, RefineDet320 and its subclasses): every activation owns `a.g`; the first consumer writes it, later ones accumulate,
    through a scratch where the kernel can only overwrite -- `emit`, `_into`, `_fold` -- and the conv / transposed conv + batch norm op of both classes:
    `conv_bn`, `conv_bn_fwd`, `conv_bn_bwd`.
The two gradient schemes stay apart: they produce different launches.  In YOLOv3 the residual input x of add(x, conv(conv(x))) shares the sum's buffer
although it has two consumers, and the conv's dgrad accumulates into it; CenterNet shares only single-consumer inputs of a sum and copies otherwise.
Nothing here allocates or touches the host once a model is built: the handlers only launch, on views of existing buffers.
"""
from __future__ import annotations

import math
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from . import ops
from .base import _Act

# one layer of a class's `specs` as the layout sees it: `wshape` the LOGICAL filter (kout, k, k, kin) -- a transposed conv stores the filter of the conv
# it is the gradient of --, `nbias` the bias length, `norm` the channels of the layer's norm (None: no norm), `stats`: the norm has moving statistics,
# `fan_in` of the He-normal initialisation, `before` / `after`: extra (name, shape) entries created in front of / behind the layer
Row = namedtuple('Row', 'name wshape nbias norm stats fan_in bias_init before after', defaults=(0., (), ()))


def param_layout(rows, chunk):
    """(pinfo, nparam, sinfo, nstat): name -> (offset, shape) of every parameter / moving statistic in the flat buffers, in creation order; every entry
    starts on a multiple of 64 elements and a filter's input channels are padded to `chunk` (host logic, no device needed)"""
    pinfo, sinfo = OrderedDict(), OrderedDict()
    off = soff = 0

    def add(name, shape):
        nonlocal off
        pinfo[name] = (off, tuple(shape))
        off += ops.pad_to(int(np.prod(shape)), 64)
    for r in rows:
        for extra, shape in r.before:
            add(extra, shape)
        kout, kh, kw, kin = r.wshape
        add(r.name + '.w', (kout, kh, kw, ops.pad_to(kin, chunk)))
        add(r.name + '.b', (r.nbias,))
        if r.norm is not None:
            add(r.name + '.gamma', (r.norm,))
            add(r.name + '.beta', (r.norm,))
            for suffix in ('.mmean', '.mvar') if r.stats else ():
                sinfo[r.name + suffix] = (soff, (r.norm,))
                soff += ops.pad_to(r.norm, 64)
        for extra, shape in r.after:
            add(extra, shape)
    return pinfo, off, sinfo, soff


def init_parameters(m, rows, seed):
    """the layout, the flat buffers (no S for a class without statistics) and the synthetic initialisation: He-normal kernels -- one draw per layer, in
    spec order --, the bias at `bias_init`, norm gamma 1 / beta 0 / moving (0, 1)"""
    m.pinfo, nparam, m.sinfo, nstat = param_layout(rows, m.chunk)
    m._alloc_flat(nparam, nstat if m.sinfo else None)
    m._cin = {r.name: r.wshape[3] for r in rows}
    g = torch.Generator().manual_seed(seed)
    for r in rows:
        m.set_param(r.name + '.w', torch.randn(*r.wshape, generator=g) * math.sqrt(2.0 / r.fan_in))
        m.param(r.name + '.b').fill_(float(r.bias_init))
        if r.norm is not None:
            m.param(r.name + '.gamma').fill_(1.0)
            if r.stats:
                m.stat(r.name + '.mvar').fill_(1.0)


def filter_table(m, rows):
    """m.wt: the dgrad-layout copy [pad(kin)][k][k][pad(kout)] of the filter of every layer of `rows`, and m._fp_batch, the one launch that refreshes them
    from P.  (The classes used to size these from the descriptor's C and the output's pitch, or from pad_to: the same numbers, checked per layer.)"""
    ch = m.chunk
    m.wt, entries = {}, []
    for r in rows:
        kout, k, _, kin = r.wshape
        kin_pad, kp = ops.pad_to(kin, ch), ops.pad_to(kout, ch)
        m.wt[r.name] = torch.zeros(kin_pad * k * k * kp, dtype=m.tdt, device=m.dev)
        entries.append((m._flat(r.name + '.w', m.P), m.wt[r.name], kout, k, k, kin_pad, kp))
    m._fp_batch = ops.FilterPrepareBatch(entries, m.DT, m.dev)


# ---------------------------------------------------------------------- shared gradient buffers (YOLOv3, RetinaNet, FCOS)
class SharedGradients:
    """`_groups`: union-find over the activations' `gid`; `g`: root gid -> the group's gradient buffer.  The class's _build starts with
    `self._groups = {}`; a source of gradients (a prediction head) enters `self.g` before `_reverse`, or is a plan op that only writes."""

    def find(self, g):
        groups = self._groups
        while groups.setdefault(g, g) != g:
            g = groups[g]
        return g

    def union(self, a, y):
        """d(a) = d(y): `a` joins y's group (a sum and its operands)"""
        self._groups[self.find(a.gid)] = self.find(y.gid)

    def grad_of(self, a):
        return self.g[self.find(a.gid)]

    def _reverse(self, io):
        """the backward order: walks self.plan in reverse and yields (op, acc).  io[kind](op) -> (the activations whose gradient the op's backward reads,
        those it writes); acc: the group of the FIRST one it writes has been written before, so this op accumulates.  Then one buffer per written group
        that has none (never the input's)."""
        written = set(self.g)
        for op in reversed(self.plan):
            reads, writes = io[op[0]](op)
            for a in reads:
                assert self.find(a.gid) in written, (op[0], a.name)
            acc = bool(writes) and self.find(writes[0].gid) in written
            written.update(self.find(a.gid) for a in writes)
            yield op, acc
        for a in self.acts.values():
            gid = self.find(a.gid)
            if gid in written and gid not in self.g and a is not self.input:
                self.g[gid] = torch.zeros(a.M, a.ld, dtype=self.tdt, device=self.dev)


# ---------------------------------------------------------------------- pre-activation ResNet + pyramid (RetinaNet, FCOS)
# (what the trunk's ops read, what they write) for SharedGradients._reverse; the stem writes no activation gradient
TRUNK_IO = {'add': lambda op: ([op[3]], []), 'resize_add': lambda op: ([op[3]], [op[2]]), 'pool': lambda op: ([op[2]], [op[1]]),
            'stem': lambda op: ([], [])}


def new_act(m, name, H, W, C):
    a = _Act(name, m.batch_size, H, W, C, ops.pad_to(C, m.chunk), m.tdt, m.dev)
    m.acts[name] = a
    return a


def conv_desc(m, name, src, cout, k, stride, ldy):
    """the descriptor of layer `name` reading every column of `src` (pad columns are zero)"""
    d = ops.conv_desc(m.batch_size, src.H, src.W, src.ld, src.ld, cout, ldy, k, stride, 1, m.CDT, m.CDT)
    m.desc[name] = d
    return d


def _add(m, a, b):
    y = new_act(m, f'sum{len(m.plan)}', a.H, a.W, a.C)
    m.union(a, y)                                              # both operands are conv outputs with this single consumer
    m.union(b, y)
    m.plan.append(('add', a, b, y))
    return y


def _resize_add(m, lat, top):
    y = new_act(m, f'total{len(m.plan)}', lat.H, lat.W, lat.C)
    m.union(lat, y)
    m.plan.append(('resize_add', lat, top, y))
    return y


def preact_resnet(m, it, block_list, normconv, stem_norm):
    """stem conv -> norm -> ReLU -> 3x3 / stride-2 max pool, then per unit [norm-ReLU-1x1, norm-ReLU-3x3, norm-ReLU-1x1] + [norm-ReLU-3x3] shortcut;
    returns the stages' outputs.  `it` yields the specs; normconv(x) appends the class's norm -> ReLU -> conv op and returns the conv's output;
    stem_norm(name, z, channels) allocates what the class's norm saves for the stem and sizes the class's scratch."""
    name, cin, cout, k, stride, nc, _ = next(it)
    d = conv_desc(m, name, m.input, cout, k, stride, ops.pad_to(cout, m.chunk))
    z = new_act(m, name + '.z', d.Ho, d.Wo, cout)
    y = new_act(m, name, d.Ho, d.Wo, cout)
    stem_norm(name, z, nc)
    m.plan.append(('stem', name, m.input, z, y))
    Hp, pt, _ = ops.same_pad(y.H, 3, 2)
    Wp, pl, _ = ops.same_pad(y.W, 3, 2)
    x = new_act(m, 'pool1', Hp, Wp, cout)
    m.plan.append(('pool', y, x, 3, 2, pt, pl))
    feats = []
    for blocks in block_list:
        for _ in range(blocks):
            branch = normconv(normconv(normconv(x)))
            x = _add(m, branch, normconv(x))
        feats.append(x)
    return feats


def fpn(m, normconv, f1, f2, f3):
    """the bilinear top-down pyramid (the SUM is handed down) and p6 / p7 -> [p3, p4, p5, p6, p7]"""
    p5 = normconv(f3)
    total4 = _resize_add(m, normconv(f2), p5)
    p4 = normconv(total4)
    total3 = _resize_add(m, normconv(f1), total4)
    p3 = normconv(total3)
    p6 = normconv(p5)
    p7 = normconv(p6)
    return [p3, p4, p5, p6, p7]


def trunk_fwd(m, op):
    """the forward launches of 'add', 'resize_add', 'pool' and the stem's CONVOLUTION (the class launches its norm behind it)"""
    kind = op[0]
    if kind == 'add':                                          # (the whole pitch: the pad columns of the 7 / 14 / 28-channel maps are zero)
        _, a, b, y = op
        ops.add2d(a.t, a.ld, b.t, b.ld, y.t, y.ld, y.M, y.ld)
    elif kind == 'resize_add':
        _, lat, top, y = op
        ops.add2d(lat.t, lat.ld, None, 0, y.t, y.ld, y.M, y.ld)
        ops.resize_bilinear_fwd(top.t, top.ld, y.t, y.ld, top.N, top.H, top.W, y.H, y.W, top.C, True)
    elif kind == 'stem':
        _, name, src, z, y = op
        ops.conv2d_fwd(m.desc[name], src.t, m._flat(name + '.w', m.Pc), m.param(name + '.b'), z.t, False)
    else:
        _, x, y, k, s, pt, pl = op
        ops.maxpool_fwd(x.t, y.t, x.N, x.H, x.W, x.C, x.ld, y.H, y.W, k, s, pt, pl)


def trunk_bwd(m, op):
    """the backward launches of 'resize_add' and 'pool' ('add' has none: its operands share its buffer; the stem's differ between the classes -- batch
    norm cancels the bias gradient, group norm does not)"""
    if op[0] == 'resize_add':
        _, lat, top, y, acc = op
        ops.resize_bilinear_bwd(m.grad_of(y), y.ld, m.grad_of(top), top.ld, top.N, top.H, top.W, y.H, y.W, top.C, acc)
    else:
        _, x, y, k, s, pt, pl = op
        ops.maxpool_bwd(x.t, y.t, m.grad_of(y), m.grad_of(x), x.N, x.H, x.W, x.C, x.ld, y.H, y.W, k, s, pt, pl)


# ---------------------------------------------------------------------- owned gradient buffers (CenterNet, RefineDet320 and its subclasses)
class OwnedGradients:
    """every activation owns its gradient buffer `a.g`; a consumer either writes it (first) or accumulates (later consumers) -- decided once, by `emit`,
    when the class builds its backward plan -- so an activation may feed any number of sums and layers"""

    def _alloc_backward(self):
        self.zg = torch.zeros(self._max_z, dtype=self.tdt, device=self.dev)             # d(pre-BN conv output): lives inside one layer
        self.scr = torch.zeros(self._max_scr, dtype=self.tdt, device=self.dev)          # an input gradient on its way to being accumulated
        self._written = set()

    def emit(self, a):
        """this consumer's contribution to d(a): first writer -> write (False), later ones -> accumulate (True); allocates a.g (never the input's)"""
        acc = id(a) in self._written
        self._written.add(id(a))
        if a.g is None and a is not self.input:
            a.g = torch.zeros(a.M, a.ld, dtype=self.tdt, device=self.dev)
        return acc

    def _into(self, a, acc):
        """destination of a kernel that can only overwrite: the gradient buffer itself (first writer) or the scratch (then added)"""
        return self.scr[: a.M * a.ld].view(a.M, a.ld) if acc else a.g

    def _fold(self, a, acc):
        if acc:
            ops.add2d(a.g, a.ld, self.scr[: a.M * a.ld].view(a.M, a.ld), a.ld, a.g, a.ld, a.M, a.ld)


def conv_bn(m, spec, src, new_y, out=None):
    """appends ('bn', name, kind, src, z, y, relu, out): conv (kind 'conv') or transposed conv ('dconv', run as the dgrad of the stride-2 conv it is
    the gradient of) + batch norm + activation `relu` (0 none | 1 ReLU | 2 leaky_relu(0.1)).  spec = (name, kind, cin, cout, k, stride, dilation, relu);
    new_y(Ho, Wo) makes the output activation; out = (tensor name, first row, width): the output goes straight into a prediction tensor."""
    name, kind, cin, cout, k, stride, dil, relu = spec
    N, ch = m.batch_size, m.chunk
    assert cin == src.C, (name, cin, src.C)
    ldz = ops.pad_to(cout, ch)
    if kind == 'conv':
        d = ops.conv_desc(N, src.H, src.W, ops.pad_to(cin, ch), src.ld, cout, ldz, k, stride, dil, m.CDT, m.CDT)
        Ho, Wo = d.Ho, d.Wo
    else:                                                       # the stride-2 conv this layer is the gradient of: [2H,2W,cout] -> [H,W,cin]
        Ho, Wo = src.H * stride, src.W * stride
        d = ops.conv_desc(N, Ho, Wo, ldz, ldz, cin, src.ld, k, stride, 1, m.CDT, m.CDT)
        assert d.Ho == src.H and d.Wo == src.W
    m.desc[name] = d
    z = _Act(name + '.z', N, Ho, Wo, cout, ldz, m.tdt, m.dev)
    m.z[name] = z
    y = new_y(Ho, Wo)
    m.bnsave[name] = (torch.zeros(cout, device=m.dev), torch.zeros(cout, device=m.dev))
    m._max_ws = max(m._max_ws, ops.bn_workspace_bytes(z.M, cout))
    m._max_z = max(m._max_z, z.M * ldz)
    m._max_scr = max(m._max_scr, src.M * src.ld)
    m.plan.append(('bn', name, kind, src, z, y, int(relu), out))
    return y


def conv_bn_fwd(m, op, training):
    _, name, lk, src, z, y, relu, out = op
    if lk == 'conv':
        ops.conv2d_fwd(m.desc[name], src.t, m._flat(name + '.w', m.Pc), m.param(name + '.b'), z.t, False)
    else:                                                       # transposed conv = dgrad of its stride-2 conv (bias: exactly 0, see _check_oracle_param)
        ops.conv2d_dgrad(m.desc[name], src.t, src.ld, m.wt[name], None, z.t, False)
    sm, si = m.bnsave[name]
    if out is None:
        dst, ldy, rpi, stride = y.t, y.ld, z.M, 0
    else:
        dst, _, stride = m._pred_view(out)
        ldy, rpi = z.C, z.H * z.W                               # a cell's NA * width outputs are contiguous rows of the prediction tensor
    ops.bn_fwd(z.t, z.M, z.C, z.ld, m.param(name + '.gamma'), m.param(name + '.beta'), m.stat(name + '.mmean'), m.stat(name + '.mvar'), sm, si,
               training, relu, dst, ldy, rpi, stride, m.ws)


def conv_bn_bwd(m, op):
    _, name, lk, src, z, y, relu, out, acc = op
    zg = m.zg[: z.M * z.ld].view(z.M, z.ld)
    sm, si = m.bnsave[name]
    if out is None:
        dy, ldy, rpi, stride, yt = y.g, y.ld, z.M, 0, (y.t if relu else None)
    else:
        dy, _, stride = m._pred_view(out, grad=True)
        ldy, rpi, yt = z.C, z.H * z.W, None
    ops.bn_bwd(z.t, yt, dy, z.M, z.C, z.ld, ldy, rpi, stride, m.param(name + '.gamma'), sm, si, relu, zg, m._flat(name + '.gamma', m.G),
               m._flat(name + '.beta', m.G), m.ws)
    # the bias feeds a batch norm: its gradient is exactly zero (only weight decay acts on it)
    if lk == 'conv':
        ops.conv2d_wgrad(m.desc[name], src.t, zg, z.ld, m._flat(name + '.w', m.G), None)
        if src is not m.input:
            ops.conv2d_dgrad(m.desc[name], zg, z.ld, m.wt[name], src.t if src.vgg else None, src.g, acc)      # (a bias + ReLU input: the consumer applies its mask)
    else:
        # filter gradient of the underlying conv with the operands swapped: its "input" is d(z), its "output gradient" the layer's input
        ops.conv2d_wgrad(m.desc[name], zg, src.t, src.ld, m._flat(name + '.w', m.G), None)
        ops.conv2d_fwd(m.desc[name], zg, m._flat(name + '.w', m.Pc), None, m._into(src, acc), False)
        m._fold(src, acc)
