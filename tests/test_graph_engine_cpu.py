"""graph.py's shared pieces on their own, on the CPU stand-in of the library (tests/mock_ops.py): the flat layout, the two backward planners (shared
gradient buffers: YOLOv3 / RetinaNet / FCOS; owned buffers: CenterNet / RefineDet320) and CenterNet's gradient sharing through the accumulate engine.
What the engines compute inside the classes is covered by tests/test_models_host_logic_cpu.py and the GPU suites."""
import torch

import mock_ops


def test_param_layout_offsets_shapes_and_extras():
    """three hand-written layers: norm + statistics, no norm, an extra entry in front (and one behind); chunk 8"""
    from odtk import graph
    rows = [graph.Row('a', (10, 3, 3, 3), 10, 10, True, 27),
            graph.Row('b', (5, 1, 1, 10), 5, None, True, 10),
            graph.Row('c', (4, 3, 3, 5), 7, 5, False, 45, 0., (('c.dw', (3, 3, 5)),), (('tail', (1,)),))]
    pinfo, nparam, sinfo, nstat = graph.param_layout(rows, 8)
    assert list(pinfo.items()) == [
        ('a.w', (0, (10, 3, 3, 8))),                          # 720 -> 768
        ('a.b', (768, (10,))), ('a.gamma', (832, (10,))), ('a.beta', (896, (10,))),
        ('b.w', (960, (5, 1, 1, 16))),                        # 80 -> 128
        ('b.b', (1088, (5,))),                                # no norm: no gamma / beta
        ('c.dw', (1152, (3, 3, 5))),                          # the extra entry comes first
        ('c.w', (1216, (4, 3, 3, 8))),                        # 288 -> 320
        ('c.b', (1536, (7,))), ('c.gamma', (1600, (5,))), ('c.beta', (1664, (5,))),
        ('tail', (1728, (1,)))]
    assert nparam == 1792
    assert list(sinfo.items()) == [('a.mmean', (0, (10,))), ('a.mvar', (64, (10,)))] and nstat == 128        # c: a norm without statistics
    assert all(off % 64 == 0 for off, _ in pinfo.values())


def test_param_layout_is_yolov3s():
    from odtk import graph
    from odtk.yolov3 import YOLOv3, layer_specs
    specs = layer_specs()
    rows = [graph.Row(name, (cout, k, k, cin), cout, cout, True, cin * k * k) for name, cin, cout, k, _, _ in specs]
    for chunk in (8, 4):
        assert graph.param_layout(rows, chunk) == YOLOv3.param_layout(specs, chunk)
    pinfo, nparam, sinfo, nstat = YOLOv3.param_layout(specs, 8)
    assert len(pinfo) == 4 * 75 and len(sinfo) == 2 * 75 and pinfo['c0.w'] == (0, (32, 3, 3, 8)) and pinfo['c0.b'] == (2304, (32,))


class _Shared:
    """the least a model has for graph.SharedGradients._reverse"""

    def __init__(self):
        from odtk import graph
        from odtk.base import _Act

        class M(graph.SharedGradients):
            pass
        m = self.m = M()
        m.tdt, m.dev, m._groups, m.g, m.plan = torch.float32, torch.device('cpu'), {}, {}, []
        m.input = _Act('input', 1, 4, 4, 3, 8, m.tdt, m.dev)
        m.acts = {'input': m.input}
        self._Act = _Act

    def conv(self, name, src):
        y = self.m.acts[name] = self._Act(name, 1, 4, 4, 8, 8, self.m.tdt, self.m.dev)
        self.m.plan.append(('conv', name, src, y))
        return y

    def add(self, a, b):
        y = self.m.acts['s'] = self._Act('s', 1, 4, 4, 8, 8, self.m.tdt, self.m.dev)
        self.m.union(a, y)
        self.m.union(b, y)
        self.m.plan.append(('add', a, b, y))
        return y


def test_shared_gradient_planner_residual_block():
    """input -> conv x -> conv a -> conv b -> add(x, b) = s -> conv c, the gradient source on c"""
    h = _Shared()
    m = h.m
    x = h.conv('x', m.input)
    b = h.conv('b', h.conv('a', x))
    s = h.add(x, b)
    c = h.conv('c', s)
    m.g[m.find(c.gid)] = torch.zeros(c.M, c.ld)
    io = {'conv': lambda op: ([op[3]], [op[2]]), 'add': lambda op: ([op[3]], [])}
    acc = {op[1]: acc for op, acc in m._reverse(io) if op[0] == 'conv'}
    assert m.find(x.gid) == m.find(b.gid) == m.find(s.gid) != m.find(m.acts['a'].gid)
    assert m.grad_of(x) is m.grad_of(b) and m.grad_of(b) is m.grad_of(s) and tuple(m.grad_of(s).shape) == (s.M, s.ld)
    assert acc == {'c': False,          # the dgrad of c writes d(s) first
                   'b': False,
                   'a': True,           # ... and the dgrad of a accumulates into the same rows: x has two consumers and still shares the sum's buffer
                   'x': False}
    assert m.find(m.input.gid) not in m.g                      # written by the planner's book-keeping, but the input never gets a buffer
    assert len({id(t) for t in m.g.values()}) == 3             # c (given), {x, b, s}, a


def test_owned_gradient_planner_two_consumers():
    from odtk import graph
    from odtk.base import _Act

    class M(graph.OwnedGradients):
        pass
    with mock_ops.installed():
        m = M()
        m.tdt, m.dev, m._max_z, m._max_scr = torch.float32, torch.device('cpu'), 64, 4 * 16 + 32
        m.input = _Act('input', 1, 2, 2, 3, 8, m.tdt, m.dev)
        a = _Act('a', 1, 2, 2, 12, 16, m.tdt, m.dev)
        m._alloc_backward()
        assert m.emit(a) is False and a.g is not None and tuple(a.g.shape) == (4, 16)
        assert m.emit(a) is True                               # the second consumer accumulates
        assert m._into(a, False) is a.g
        scr = m._into(a, True)
        assert scr.data_ptr() == m.scr.data_ptr() and tuple(scr.shape) == (4, 16) and scr.numel() < m.scr.numel()
        assert m.emit(m.input) is False and m.input.g is None  # the input never gets a buffer
        a.g.fill_(1.0); scr.fill_(2.0)
        m._fold(a, False)
        assert float(a.g.sum()) == 64.0
        m._fold(a, True)
        assert float(a.g.sum()) == 192.0


def _centernet_backward_plan(**config):
    """CenterNet._build_backward on a hand-made plan: input -> u -> v, s = add(v, u), three heads on s.  v feeds only the sum, u also feeds v's layer"""
    from odtk.base import _Act
    from odtk.centernet import CenterNet
    m = object.__new__(CenterNet)
    m.tdt, m.dev, m.config, m._max_z, m._max_scr, m.plan = torch.float32, torch.device('cpu'), config, 64, 64, []
    m.input = _Act('input', 1, 2, 2, 3, 8, m.tdt, m.dev)

    def layer(name, src, C=8):
        y = _Act(name, 1, 2, 2, C, 8 if C == 8 else C, m.tdt, m.dev)
        m.plan.append(('bn', name, 'conv', src, _Act(name + '.z', 1, 2, 2, C, 8, m.tdt, m.dev), y, 1, None))
        return y
    u = layer('u', m.input)
    v = layer('v', u)
    s = _Act('s', 1, 2, 2, 8, 8, m.tdt, m.dev)
    m.plan.append(('add', [v, u], s))
    m.kp_act, m.off_act, m.size_act = layer('kp', s, 3), layer('off', s, 2), layer('size', s, 2)
    m.keypoints, m.offset, m.size = m.kp_act.t.view(1, 2, 2, 3), m.off_act.t.view(1, 2, 2, 2), m.size_act.t.view(1, 2, 2, 2)
    m._build_backward(1, m.tdt, m.dev)
    return m, u, v, s


def test_centernet_shares_the_gradient_of_single_consumer_sum_inputs():
    with mock_ops.installed():
        m, u, v, s = _centernet_backward_plan()
        assert v.g is s.g and m.shared_grads == 1              # d(v) = d(s) exactly: no copy, no launch
        assert u.g is not s.g and u.g.data_ptr() != s.g.data_ptr() and tuple(u.g.shape) == (u.M, u.ld)         # two consumers: its own buffer
        add = [op for op in m.bplan if op[0] == 'add']
        assert len(add) == 1 and [(a.name, acc) for a, acc in add[0][1]] == [('u', False)]       # the sum writes d(u) first; v's layer accumulates
        assert [op[-1] for op in m.bplan if op[0] == 'bn' and op[1] == 'v'] == [True]
        assert [op[-1] for op in m.bplan if op[0] == 'bn' and op[1] in ('kp', 'off', 'size')] == [False, True, True]
        m, u, v, s = _centernet_backward_plan(share_sum_gradients=False)
        assert m.shared_grads == 0 and v.g is not s.g and v.g.data_ptr() != s.g.data_ptr() and tuple(v.g.shape) == (v.M, v.ld)
        add = [op for op in m.bplan if op[0] == 'add']
        assert [(a.name, acc) for a, acc in add[0][1]] == [('v', False), ('u', False)]
