"""CIST-GCN on MI355X: the `nn.Module` surface of the reference model
(human_motion_prediction/models/CISTGCN/CISTGCN.py:478-597) with the arithmetic on hand-written
gfx950 kernels (cistgcn_amd/csrc, called through cistgcn_amd/ops.py).

What is kept from the reference, because its callers depend on it:
class name `CISTGCN`, ctor `(arch, learn)`, `forward(x: (B,T_in,V,3)) -> (pred: (B,T_out,V,3),)`,
every `state_dict` key / shape, the init (same RNG consumption order, so the same seed gives the
same weights), and the interpretation attributes written by each forward
(`st_gcnns.{i}.{dsgn,tsgn}.Adj`, `.w1`, `.w2`, `context_layer.{joints,displacements,seq_joints,
seq_joints_n,seq_joints_dims}`).

The torch leaf modules below (`nn.Conv2d`, `nn.BatchNorm2d`, ...) are parameter holders only; their
`forward` is never called.  There is no CPU path: tensors must live on the HIP device.
"""
from types import SimpleNamespace

import torch
import torch.nn as nn

from ... import ops
from ..layers.SE import SELayer1d, SELayer2d

# Dropout site ids and the salts of ops.draw_augmentation share the salt field of the seed hash: the ids stay below the first draw salt
_DRAW_SALT = ops._lib.LIMITS["CG_DRAW_SALT"]


class Stage(nn.Module):
    """Numbered parameter slots of one reference `nn.Sequential` (gaps = parameter-free steps)."""

    def __init__(self, **slots):
        super().__init__()
        for k, m in slots.items():
            self.add_module(k.lstrip("s"), m)

    def __getitem__(self, i):
        return self._modules[str(i)]


def _conv(cin, cout, k=1, bias=False, **kw):
    return nn.Conv2d(cin, cout, k, bias=bias, **kw)


def _init_small(root, gain, convs):
    """Reference init passes: Map2Adj (CISTGCN.py:175-181, gain .05, convs too) and the model-level
    one (:559-565, gain .1, Linear + PReLU only)."""
    for m in root.modules():
        if isinstance(m, nn.Linear):
            nn.init.xavier_uniform_(m.weight, gain=gain)
        if convs and isinstance(m, (nn.Conv2d, nn.Conv1d)):
            nn.init.xavier_normal_(m.weight, gain=gain)
        if isinstance(m, nn.PReLU):
            nn.init.constant_(m.weight, 0.25)


class Map2Adj(nn.Module):
    """Parameters of the interpretability attention map (CISTGCN.py:127-181)."""

    def __init__(self, cin, time_dim, joints_dim, domain):
        super().__init__()
        mid = cin // 2
        def tower(kernel, out):
            return Stage(s0=_conv(cin, mid), s1=nn.BatchNorm2d(mid), s2=nn.PReLU(), s3=_conv(mid, mid, kernel),
                         s4=nn.BatchNorm2d(mid), s6=_conv(mid, out))
        self.time_compress = tower((time_dim, 1), time_dim)
        self.joint_compress = tower((1, joints_dim), joints_dim)
        ch = joints_dim if domain == "space" else time_dim
        self.expansor = Stage(s0=_conv(ch, ch), s1=nn.BatchNorm2d(ch), s3=nn.PReLU(), s4=_conv(ch, ch))
        for part in (self.time_compress, self.joint_compress, self.expansor):
            _init_small(part, 0.05, True)


class GraphWeights(nn.Module):
    """`gcn` slot of a domain layer.  Interpretable layers get their adjacency per sample from
    Map2Adj and own no parameter; otherwise a batch-shared A (CISTGCN.py:104-120)."""

    def __init__(self, time_dim, joints_dim, domain, interpretable):
        super().__init__()
        if not interpretable:
            n, s = (time_dim, joints_dim) if domain == "time" else (joints_dim, time_dim)
            self.A = nn.Parameter(torch.empty(n, s, s).uniform_(-1.0 / s ** 0.5, 1.0 / s ** 0.5))


class DomainLayer(nn.Module):
    """Parameters of one Domain_GCNN_layer (CISTGCN.py:208-257); kernel size is [1,1] in every
    instantiation of the reference (:524,:553), so `tcn.0` is a channel-mixing matrix."""

    def __init__(self, cin, cout, time_dim, joints_dim, domain, interpretable):
        super().__init__()
        self.domain, self.interpretable = domain, bool(interpretable)
        self.gcn = GraphWeights(time_dim, joints_dim, domain, interpretable)
        self.tcn = Stage(s0=_conv(cin, cout, bias=True), s1=nn.BatchNorm2d(cout))
        self.residual = Stage(s0=_conv(cin, cout, bias=True), s1=nn.BatchNorm2d(cout)) if cin != cout else nn.Identity()
        self.map_to_adj = Map2Adj(cin, time_dim, joints_dim, domain) if interpretable else nn.Identity()
        self.prelu = nn.PReLU()


class DSTDBlock(nn.Module):
    """Parameters of one DSTD_GC block (CISTGCN.py:289-358)."""

    def __init__(self, cin, cout, interpretable, time_dim, joints_dim, reduction):
        super().__init__()
        self.dsgn = DomainLayer(cin, cout, time_dim, joints_dim, "space", interpretable)
        self.tsgn = DomainLayer(cin, cout, time_dim, joints_dim, "time", interpretable)
        self.compressor = Stage(s0=_conv(2 * cout, cout), s1=nn.BatchNorm2d(cout), s2=nn.PReLU(),
                                s3=SELayer2d(cout, reduction=reduction))
        self.residual = Stage(s0=_conv(cin, cout, bias=True), s1=nn.BatchNorm2d(cout)) if cin != cout else nn.Identity()
        mid = max(1, cout // 2)
        self.global_norm = nn.BatchNorm2d(cin)
        def gate_conv():
            return Stage(s0=_conv(cin, mid, (time_dim, 1)), s1=nn.BatchNorm2d(mid), s3=nn.PReLU(),
                         s4=_conv(mid, cout, (1, joints_dim)), s5=nn.BatchNorm2d(cout), s7=nn.PReLU())
        def gate_map():
            return Stage(s0=nn.Linear(cout + 2 + 2 * time_dim, cout, bias=False), s1=nn.BatchNorm1d(cout), s3=nn.PReLU(),
                         s4=nn.Linear(cout, cout, bias=False))
        self.conv_s, self.conv_t = gate_conv(), gate_conv()
        self.map_s, self.map_t = gate_map(), gate_map()
        self.prelu1 = Stage(s0=nn.BatchNorm2d(cout), s1=nn.PReLU())
        self.prelu2 = Stage(s0=nn.BatchNorm2d(cout), s1=nn.PReLU())


class FPN(nn.Module):
    """Parameters of one time-extrapolator block (CISTGCN.py:38-72)."""

    def __init__(self, cin, cout, k):
        super().__init__()
        if k != 3:
            raise ValueError("txc_kernel_size %d is not supported by the MI355X path (reference YAMLs use 3)" % k)
        for i, d in enumerate((1, 2, 3)):
            self.add_module("block%d" % (i + 1), Stage(s0=_conv(cin, cout, 3, bias=True, padding=d, dilation=d),
                                                       s1=nn.BatchNorm2d(cout), s3=nn.PReLU()))
        self.compress = _conv(3 * cout + cin, cout, bias=True)


class ContextLayer(nn.Module):
    """Parameters of the context branch (CISTGCN.py:394-461)."""

    def __init__(self, hidden, out_seq, joints, reduction):
        super().__init__()
        def ctx_conv(k):
            return Stage(s0=_conv(1, hidden, k), s1=nn.BatchNorm2d(hidden), s2=nn.PReLU())
        self.context_conv1, self.context_conv2, self.context_conv3 = ctx_conv(1), ctx_conv((out_seq, 1)), ctx_conv(1)
        def head():
            return Stage(s0=nn.Linear(hidden, out_seq, bias=False), s2=nn.PReLU())
        self.map1, self.map2, self.map3 = head(), head(), head()
        self.fmap_s = Stage(s0=nn.Linear(3 * out_seq, joints, bias=False), s1=nn.BatchNorm1d(joints))
        self.fmap_t = Stage(s0=nn.Linear(3 * out_seq, out_seq, bias=False), s1=nn.BatchNorm1d(out_seq))
        self.norm_map = Stage(s0=nn.Conv1d(out_seq, out_seq, 1, bias=False), s1=nn.BatchNorm1d(out_seq), s3=nn.PReLU(),
                              s4=SELayer1d(out_seq, reduction=reduction),
                              s5=nn.Conv1d(out_seq, out_seq, 1, bias=False), s6=nn.BatchNorm1d(out_seq), s8=nn.PReLU())
        self.fconv = Stage(s0=_conv(1, 3), s1=nn.BatchNorm2d(3), s2=nn.PReLU(), s3=_conv(3, 3), s4=nn.BatchNorm2d(3), s5=nn.PReLU())
        self.SE = SELayer2d(out_seq, reduction=reduction)


# ---- linear maps as contractions (weights are viewed, never copied) ------------------------------
# Each helper returns (y, stats): stats are the f64 per-channel sums of y from the contraction epilogue
# when `stats=True` (a train-mode BatchNorm follows), else None.
def _pointwise(x, conv, stats=False):
    """1x1 convolution over the channel axis of a 3-D or 4-D (possibly strided) tensor."""
    w = conv.weight.view(conv.out_channels, conv.in_channels)
    if x.dim() == 4 and x.shape[0] * x.shape[2] * x.shape[3] >= _PWM_MIN_POSITIONS and ops.pointwise_maps_ok(x, [w]):
        # long position axis: the stacked pointwise kernel with one map (x, dy read once each backward; the generic contraction split the
        # weight gradient of a 3-channel map over 265 workgroups with atomics: 41 us for 3.4 MB)
        return ops.pointwise_maps(x, [w], stats, biases=[conv.bias])[0]
    spec = "oc,bchw->bohw" if x.dim() == 4 else "oc,bcv->bov"
    bl = "o" if conv.bias is not None else None
    return ops.contract_stats(spec, w, x, conv.bias, bl) if stats else (ops.contract(spec, w, x, conv.bias, bl), None)


_PWM_MIN_POSITIONS = 32768     # B * H * W from which single 1x1 maps take the stacked kernel


def _collapse_rows(x, conv, stats=False):
    """(H,1) convolution that spans the whole axis 2: (B,C,H,W) -> (B,O,1,W)."""
    w = conv.weight.view(conv.out_channels, conv.in_channels, x.shape[2])
    y, st = ops.contract_stats("och,bchw->bow", w, x) if stats else (ops.contract("och,bchw->bow", w, x), None)
    return y.view(y.shape[0], y.shape[1], 1, y.shape[2]), st


def _collapse_cols(x, conv, stats=False):
    """(1,W) convolution that spans the whole axis 3: (B,C,H,W) -> (B,O,H,1)."""
    w = conv.weight.view(conv.out_channels, conv.in_channels, x.shape[3])
    y, st = ops.contract_stats("ocw,bchw->boh", w, x) if stats else (ops.contract("ocw,bchw->boh", w, x), None)
    return y.view(y.shape[0], y.shape[1], y.shape[2], 1), st


def _linear(x, lin, stats=False):
    return ops.contract_stats("oi,bi->bo", lin.weight, x) if stats else (ops.contract("oi,bi->bo", lin.weight, x), None)


# ---- the same maps as contraction items for ops.contract_many (one launch per stage) ---------------
def _pw_item(x, conv, stats):
    w = conv.weight.view(conv.out_channels, conv.in_channels)
    spec = "oc,bchw->bohw" if x.dim() == 4 else "oc,bcv->bov"
    return (spec, w, x, conv.bias, "o" if conv.bias is not None else None, "o" if stats else None), None


def _rows_item(x, conv, stats):
    w = conv.weight.view(conv.out_channels, conv.in_channels, x.shape[2])
    return ("och,bchw->bow", w, x, None, None, "o" if stats else None), (lambda y: y.view(y.shape[0], y.shape[1], 1, y.shape[2]))


def _cols_item(x, conv, stats):
    w = conv.weight.view(conv.out_channels, conv.in_channels, x.shape[3])
    return ("ocw,bchw->boh", w, x, None, None, "o" if stats else None), (lambda y: y.view(y.shape[0], y.shape[1], y.shape[2], 1))


def _lin_item(x, lin, stats):
    return ("oi,bi->bo", lin.weight, x, None, None, "o" if stats else None), None


def _run_items(items):
    """items: list of (contraction item, view-fixup) -> list of (y, channel sums)"""
    outs = ops.contract_many([it for it, _ in items])
    return [((post(y) if post is not None else y), st) for (y, st), (_, post) in zip(outs, items)]


class CISTGCN(nn.Module):
    """
    Shape:
        - Input:  (N, T_in, V, 3) float32 poses on the HIP device
        - Output: 1-tuple with (N, T_out, V, 3)
    """

    def __init__(self, arch, learn):
        super().__init__()
        p = arch.model_params
        self.clipping = p.clipping
        self.n_input, self.n_output, self.n_joints = p.input_n, p.output_n, p.joints
        self.n_txcnn_layers = p.n_txcnn_layers
        self.txc_kernel_size = [p.txc_kernel_size] * 2
        self.input_gcn, self.output_gcn = p.input_gcn, p.output_gcn
        self.reduction, self.hidden_dim = p.reduction, p.hidden_dim
        self.dropout = float(learn.dropout)
        self.in_ch = 10
        self.fused_domain = True     # False: graph product and channel mix as two generic contractions
        self.staged = True           # True: same-depth ops of a block's parallel branches share one launch
        # the switches below are for tests, which pin one plan against another (tests/checks.py::build_pair, test_gpu_parity.py)
        self.fused_tail = True       # everything behind the tcn convolutions of a block as phase kernels (ops.dstd_tail)
        self.fused_adj = True        # seed, expansor and adjacency of both Map2Adj towers as phase kernels (ops.map2adj_tail)
        self.fused_maps = True       # the first-level maps of a block (towers, gates, residual maps) and of the context heads stacked
        self.fused_defer = True      # BatchNorm + PReLU of the first tower level applied by the collapsing kernels on load
        self.stack_min_elements = 1 << 21      # block inputs smaller than this keep one contraction per first-level map
        # The reference edits the config lists in place (CISTGCN.py:514-517,548); copies are used here
        # so that one `opt` can build several models.
        widths = [self.in_ch] + list(p.input_gcn.model_complexity) + [self.in_ch]
        widths_o = [3] + list(p.output_gcn.model_complexity)
        T, V, To = self.n_input, self.n_joints, self.n_output

        self.st_gcnns = nn.ModuleList()
        self.txcnns = nn.ModuleList()
        self.se = nn.ModuleList()
        self.in_conv = nn.ModuleList()
        self.context_layer = nn.ModuleList()
        self.trans = nn.ModuleList()
        for i in range(len(widths) - 1):
            self.st_gcnns.append(DSTDBlock(widths[i], widths[i + 1], p.input_gcn.interpretable[i], T, V, self.reduction))
        self.context_layer = ContextLayer(self.hidden_dim, To, V, self.reduction)
        self.txcnns.append(FPN(T, To, p.txc_kernel_size))
        for _ in range(1, self.n_txcnn_layers):
            self.txcnns.append(FPN(To, To, p.txc_kernel_size))
        self.prelus = nn.ModuleList(nn.PReLU() for _ in range(self.n_txcnn_layers))
        self.dim_conversor = Stage(s0=_conv(self.in_ch, 3), s1=nn.BatchNorm2d(3), s2=nn.PReLU(), s3=_conv(3, 3), s4=nn.PReLU(3))
        self.st_gcnns_o = nn.ModuleList()
        for i in range(len(widths_o) - 1):
            # the output block runs on (N,3,V,T_out): "time" axis = joints, "joint" axis = frames (:553)
            self.st_gcnns_o.append(DSTDBlock(widths_o[i], widths_o[i + 1], p.output_gcn.interpretable[i], V, To, self.reduction))
        for part in (self.st_gcnns_o, self.st_gcnns, self.txcnns):
            _init_small(part, 0.1, False)
        self._site = 0
        self.backward_cut = None      # (input block index, fn): the step runtime cuts the autograd graph behind that block
        self.act_trace = None         # dict: PReLU module -> (output, post-activation addend) of the last forward (diagnostics)
        self.drop_trace = None        # dict: module naming a dropout site (the BatchNorm in front of it, else the PReLU behind it) -> site id of the last forward (diagnostics)
        self.branch_streams = False   # True: independent branches of a block run on forked HIP streams (runtime.GraphedStep)
        self._streams, self._next_stream = [], 0

    # ---- fork / join of independent branches -----------------------------------------------------
    def _parallel(self, thunks, inputs):
        """Evaluate independent sub-graphs.  With `branch_streams`, all but the last are issued on side streams forked
        from the current stream and joined before returning (the last one stays on the current stream); captured in a HIP
        graph they become parallel branches, and autograd replays each backward on its forward stream, so the small
        kernels of the two branches overlap in both directions.  Fork and join are the only cross-stream edges: every
        tensor that crosses is produced before the fork or consumed after the join, which is also what keeps the caching
        allocator's per-stream reuse safe without record_stream."""
        if not (self.branch_streams and inputs[0].is_cuda) or len(thunks) < 2:
            return [t() for t in thunks]
        cur = torch.cuda.current_stream()
        while len(self._streams) < len(thunks) - 1:
            self._streams.append(torch.cuda.Stream(device=inputs[0].device))
        results = []
        for t, s in zip(thunks[:-1], self._streams):
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                results.append(t())
        results.append(thunks[-1]())
        for s in self._streams[:len(thunks) - 1]:
            cur.wait_stream(s)
        return results

    # ---- fused row op with per-call dropout site id -------------------------------------------
    def _na(self, x, bn=None, prelu=None, drop=False, **kw):
        """x is a tensor or the (y, channel-sums) pair returned by the linear-map helpers."""
        return self._na_many([dict(x=x, bn=bn, prelu=prelu, drop=drop, **kw)])[0]

    def _lin(self, fn, x, layer, bn=True):
        """linear map `fn` followed (bn=True) by a BatchNorm: ask the kernel for channel sums in train mode"""
        return fn(x, layer, stats=bn and self.training)

    # ---- Map2Adj.forward, CISTGCN.py:183-189 ----------------------------------------------------
    def _adjacency(self, layer, x):
        m = layer.map_to_adj
        B, _, T, V = x.shape

        def tower(t, collapse):
            h = self._na(self._lin(_pointwise, x, t[0]), bn=t[1], prelu=t[2])
            h = self._na(self._lin(collapse, h, t[3]), bn=t[4], drop=True)
            return _pointwise(h, t[6])[0]

        q, s = self._parallel([lambda: tower(m.time_compress, _collapse_rows), lambda: tower(m.joint_compress, _collapse_cols)], [x])
        q, s = q.view(B, T, V), s.view(B, V, T)                       # q[b,tau,v], s[b,v,t]
        if layer.domain == "space":
            o = ops.contract("bvt,bxv->bvtx", s, q)                  # o[b,v,t,tau] = s[b,v,t] q[b,tau,v]
        else:
            o = ops.contract("bvt,btw->btvw", s, q)                  # o[b,t,v,w]  = s[b,v,t] q[b,t,w]
        e = m.expansor
        h = self._na(self._lin(_pointwise, o, e[0]), bn=e[1], drop=True, prelu=e[3])
        return _pointwise(h, e[4])[0]

    def _fused_stage_ok(self, conv):
        """The fused graph-product + channel-mix kernel takes layers up to 128 channels (its LDS image); wider layers (any
        `model_complexity` is legal in the reference) go through the two generic contractions."""
        return self.fused_domain and conv.in_channels <= 128 and conv.out_channels <= 128

    # ---- Domain_GCNN_layer.forward, CISTGCN.py:259-269 -------------------------------------------
    def _domain(self, layer, xn):
        res = xn if isinstance(layer.residual, nn.Identity) else self._na(self._lin(_pointwise, xn, layer.residual[0]), bn=layer.residual[1])
        conv = layer.tcn[0]
        if layer.interpretable:
            adj = self._adjacency(layer, xn)
            layer.Adj = adj
            if self._fused_stage_ok(conv):
                w = conv.weight.view(conv.out_channels, conv.in_channels)
                y = ops.stgcn_domain(xn, adj, w, conv.bias, 0 if layer.domain == "space" else 1, self.training)
            else:
                spec = "bctv,bvtq->bcqv" if layer.domain == "space" else "bctv,btvw->bctw"
                y = self._lin(_pointwise, ops.contract(spec, xn, adj), conv)
        else:
            layer.Adj = xn
            spec = "bctv,vtq->bcqv" if layer.domain == "space" else "bctv,tvw->bctw"
            y = self._lin(_pointwise, ops.contract(spec, xn, layer.gcn.A), conv)
        return self._na(y, bn=layer.tcn[1], drop=True, add=res, prelu=layer.prelu)

    # ---- gate path of DSTD_GC.forward, CISTGCN.py:378-384 ----------------------------------------
    def _gate(self, conv, mp, xn, stats):
        h = self._na(self._lin(_collapse_rows, xn, conv[0]), bn=conv[1], drop=True, prelu=conv[3])
        h = self._na(self._lin(_collapse_cols, h, conv[4]), bn=conv[5], drop=True, prelu=conv[7])
        h = ops.cat_channels([h.view(h.shape[0], -1), stats])
        h = self._na(self._lin(_linear, h, mp[0]), bn=mp[1], drop=True, prelu=mp[3])
        return _linear(h, mp[4])[0]

    # ---- DSTD_GC.forward, CISTGCN.py:373-390 ------------------------------------------------------
    def _block(self, m, x):
        xn = self._na(x, bn=m.global_norm)
        stats = ops.dstd_stats(xn)                      # computed once; the reference evaluates it twice (:377,:379)
        m.w1, m.w2, x1, x2 = self._parallel([lambda: self._gate(m.conv_s, m.map_s, xn, stats),
                                             lambda: self._gate(m.conv_t, m.map_t, xn, stats),
                                             lambda: self._domain(m.dsgn, xn), lambda: self._domain(m.tsgn, xn)], [xn, stats])
        a = self._na(x1, pre=m.w1, bn=m.prelu1[0], prelu=m.prelu1[1])
        b = self._na(x2, pre=m.w2, bn=m.prelu2[0], prelu=m.prelu2[1])
        c = m.compressor
        h = self._na(self._lin(_pointwise, ops.cat_channels([a, b]), c[0]), bn=c[1], prelu=c[2])
        gate = ops.se_gate(ops.mean_bc(h), c[3].w1, c[3].w2)
        res = xn if isinstance(m.residual, nn.Identity) else self._na(self._lin(_pointwise, xn, m.residual[0]), bn=m.residual[1])
        return self._na(h, pre=gate, add=res, add_post=True)

    # ---- the same block with horizontal fusion ---------------------------------------------------------
    def _na_many(self, calls):
        """calls: dicts for ops.norm_act (x may be a (tensor, sums) pair); adds train flag, dropout and site ids.  A call numbers its
        site here, from the counter, unless it brings its `salt` (the staged block: ids from `_block_sites`, which traced them)."""
        out = []
        for kw in calls:
            kw = dict(kw)
            drop = kw.pop("drop", False)
            if kw.get("salt") is None:
                self._site += 1
                assert self._site < _DRAW_SALT, "dropout site ids must stay below the salts of the augmentation draws"
                kw["salt"] = self._site
                if drop and self.drop_trace is not None:
                    self.drop_trace[kw.get("bn") if kw.get("bn") is not None else kw.get("prelu")] = self._site
            kw.update(train=self.training, drop_p=self.dropout if drop else 0.0)
            out.append(kw)
        ys = ops.norm_act_many(out)
        if self.act_trace is not None:
            # branch record of every PReLU (its output, and the addend when that is added behind the activation):
            # lets a checker replay another implementation of the network on the very same branches
            for kw, y in zip(out, ys):
                if kw.get("prelu") is not None:
                    y = y[0] if isinstance(y, tuple) else y
                    add = kw.get("add") if kw.get("add_post") else None
                    self.act_trace[kw["prelu"]] = (y.detach(), add.detach() if add is not None else None)
        return ys

    @staticmethod
    def _map_groups(x, ws):
        """index groups of the 1x1 maps `ws` of x that `ops.pointwise_maps` takes in one launch each; None when one of them does not
        fit the kernel at all.  The limits are the kernel's (CG_PWM_MAXN maps and CG_PWM_MAXROWS stacked output rows per launch,
        include/cistgcn_hip.h; `ops.pointwise_maps_ok` checks the same two), every map rounded up to its 16-row tiles."""
        lim = ops._lib.LIMITS
        max_maps, max_rows = lim["CG_PWM_MAXN"], lim["CG_PWM_MAXROWS"]
        tile = 16                      # output rows of one matrix-core tile of csrc/tower_maps.hip (the header names no constant for it)
        groups, rows = [], 0
        for i, w in enumerate(ws):
            if not ops.pointwise_maps_ok(x, [w]):
                return None
            r = (w.shape[0] + tile - 1) // tile * tile
            if not groups or rows + r > max_rows or len(groups[-1]) == max_maps:
                groups.append([])
                rows = 0
            groups[-1].append(i)
            rows += r
        return groups

    def _block_staged(self, m, x):
        """DSTD_GC.forward (CISTGCN.py:373-390) with the gate paths (:378-384), the four Map2Adj towers (:183-189) and
        the two domain layers (:259-269) advanced in lock-step: every stage is one contraction launch or one row-kernel
        launch for all branches instead of one launch per branch and op.  Which kernels a stage launches is decided once,
        in `_plan_block`; which dropout site each of them draws from, in `_block_sites`."""
        if not (m.dsgn.interpretable and m.tsgn.interpretable):
            return self._block(m, x)
        x_in = x[0] if isinstance(x, tuple) else x       # (tensor, f64 channel sums) from the previous block's tail in train mode
        p = self._plan_block(m, x_in)
        s = self._block_sites(m)
        br = self._branches(m, p)
        xs = self._stage_input(m, p, s, x)
        self._stage_maps(p, br, xs)                      # 1. every first-level map of xn
        self._stage_map_tails(p, s, br, xs)              # 2. their BatchNorm / PReLU tails
        self._stage_collapse(p, br)                      # 3. collapsing convolutions
        if p.gate_fused:                                 # 4. BatchNorm tails, 5. gate Linear + last tower maps
            self._stage_mid(m, p, s, br, xs)
        else:
            self._stage_mid_chain(p, s, br, xs)
        adj = self._stage_adjacency(m, p, s, br)         # 6. rank-1 products, 7. gate output Linear + expansor
        return self._stage_graph_tail(m, p, s, br, xs, adj)      # 8. graph product + channel mix, then BN + residual + PReLU

    def _plan_block(self, m, x_in):
        """Every route decision of one call of the staged block, taken before its first launch from the block's modules, the shape and
        contiguity of its input, the model switches and the mode.  Every tensor a predicate is asked about further down is a fresh
        contiguous output of a kernel, or an alias of the normalised input (contiguous wherever a stacked kernel is chosen for it), so
        its shape says all the predicate reads: a `meta` probe stands in for it.  Left to the tail stage: whether the tcn outputs came
        with their channel sums (a generic contraction that splits K has none) and whether the two residual aliases are one tensor."""
        p = SimpleNamespace(tr=self.training)
        B, _, T, V = x_in.shape
        p.B, p.T, p.V = B, T, V
        p.has_res = not isinstance(m.dsgn.residual, nn.Identity)
        p.has_bres = not isinstance(m.residual, nn.Identity)
        p.fused_in = ops.block_input_ok(x_in)
        towers = [t for d in (m.dsgn, m.tsgn) for t in (d.map_to_adj.time_compress, d.map_to_adj.joint_compress)]
        p.tower_w = [t[0].weight.view(t[0].out_channels, t[0].in_channels) for t in towers]
        # the four tower convolutions read the block input in one pass, forward and backward (csrc/tower_maps.hip)
        # (both stackings below pay off once the block input is worth the two or three extra small launches: measured break-even
        # between the B=16 / C=8 and the B=256 / C=64 workloads)
        big = x_in.numel() >= self.stack_min_elements
        p.stacked = big and self.fused_maps and all(t[0].bias is None for t in towers) and ops.pointwise_maps_ok(x_in, p.tower_w)
        # the two gate paths start with the same (T,1) convolution shape on the same input: one convolution of the stacked weights
        # (the block input travels once instead of twice, forward and in both gradients)
        cs, ct = m.conv_s[0], m.conv_t[0]
        p.gates = big and self.fused_maps and cs.weight.shape == ct.weight.shape and cs.bias is None and ct.bias is None
        p.rows_gate = p.gates and 2 * cs.out_channels <= 64 and ops.collapse_rows_ok(x_in, cs.weight.view(cs.out_channels, cs.in_channels, -1))
        # the residual maps of a block that changes its width (1x1 convolutions WITH bias, CISTGCN.py:246-254 / :357-365) read the block
        # input in one pass per group as well (a group: up to 128 stacked output rows)
        res = ([d.residual for d in (m.dsgn, m.tsgn)] if p.has_res else []) + ([m.residual] if p.has_bres else [])
        p.res_convs, p.res_bns = [r[0] for r in res], [r[1] for r in res]
        p.res_w = [c.weight.view(c.out_channels, c.in_channels) for c in p.res_convs]
        p.res_groups = self._map_groups(x_in, p.res_w) if (big and self.fused_maps and res) else None
        # the residual maps with their BatchNorm as one operator per group, like the towers: backward is one reduction pass and the
        # pointwise backward undoing the BatchNorm on load (as two operators: 229 us of cg_norm_act_bwd on the 10 -> 64 block)
        p.res_fused = p.res_groups is not None and all(ops.tower_maps_ok(x_in, [p.res_w[i] for i in grp], [None] * len(grp)) for grp in p.res_groups)
        # first level of the four towers with its BatchNorm + PReLU as one operator: backward never stores the gradient in front of
        # the BatchNorm (the pointwise backward undoes BatchNorm and PReLU while loading)
        p.tower_fused = p.stacked and ops.tower_maps_ok(x_in, p.tower_w, [t[2] for t in towers])

        def collapse_ok(k, t):       # tower k's (T,1) or (1,V) convolution as a whole-sample kernel (csrc/collapse_rows.hip)
            probe = torch.empty((B, t[0].out_channels, T, V), device="meta")      # the shape of its first-level map, nothing allocated
            w = t[3].weight.view(t[3].out_channels, t[3].in_channels, -1)
            return big and t[3].bias is None and (ops.collapse_rows_ok(probe, w) if k % 2 == 0 else ops.collapse_cols_ok(probe, w))
        p.collapse = [collapse_ok(k, t) for k, t in enumerate(towers)]
        # ... and, when every map goes into a whole-sample collapsing kernel, the BatchNorm + PReLU themselves move into that
        # kernel's load path: the four activated (B, C/2, T, V) maps are never stored (unless branch records are asked for: `want_tap`)
        p.defer = p.tower_fused and self.fused_defer and all(p.collapse)
        p.adj_fused = self.fused_adj and T <= 64 and V <= 64
        # the middle of the block as one operator (csrc/block_mid.hip): only between the whole-sample collapsing kernels and the two fused tails
        mid_on = big and p.adj_fused
        g4s, g4t = m.conv_s[4], m.conv_t[4]
        heads = (m.conv_s[7], m.conv_t[7], m.map_s[3], m.map_t[3])
        p.mid_g = (mid_on and p.rows_gate and g4s.bias is None and g4t.bias is None
                   and tuple(g4s.kernel_size) == (1, V) and tuple(g4t.kernel_size) == (1, V) and g4s.out_channels == g4t.out_channels
                   and ops.gate_head_ok(B, g4s.out_channels, 2 + 2 * T, heads)
                   and ops.block_mid_ok(B, [(0, cs.out_channels, V, g4s.out_channels, m.conv_s[3]), (0, cs.out_channels, V, g4t.out_channels, m.conv_t[3])]))
        # the (1,V) convolution leaves (B, Cg, 1, 1): everything of the two gate paths behind it in ONE launch (csrc/gate_head.hip)
        p.gate_fused = p.mid_g or (tuple(g4s.kernel_size) == (1, V) and ops.gate_head_ok(B, g4s.out_channels, 2 + 2 * T, heads))
        # a collapsed tower map is (B, O, 1, V) behind the (T,1) convolution and (B, O, T, 1) behind the (1,V) one
        p.mid_t = (mid_on and p.gate_fused and all(p.collapse) and all(t[6].bias is None for t in towers)
                   and ops.block_mid_ok(B, [(1, t[3].out_channels, T if k % 2 else V, t[6].out_channels, None) for k, t in enumerate(towers)]))
        p.stage_fused = [self._fused_stage_ok(d.tcn[0]) for d in (m.dsgn, m.tsgn)]
        # everything behind the two tcn convolutions in five phase launches (csrc/dstd_tail.hip)
        p.tail_fused = self.fused_tail and m.compressor[0].out_channels <= 64
        return p

    def _block_sites(self, m):
        """The dropout-site ids of one block by name, counted from `self._site` in the order the row-kernel chain numbers them, which
        `self._site` is advanced past.  The ids belong to the block's modules, not to the route: a fused kernel draws its masks from
        the ids of the row kernels it replaces (dropout-free ones included), so later layers draw the same masks on every route
        (checks.check_block_sites_are_route_independent).  `drop_trace` gets the fourteen sites that do drop."""
        def take(n):
            ids = tuple(range(self._site + 1, self._site + 1 + n))
            self._site += n
            assert self._site < _DRAW_SALT, "dropout site ids must stay below the salts of the augmentation draws"
            return ids
        doms = (m.dsgn, m.tsgn)
        s = SimpleNamespace()
        s.global_norm, = take(1)
        s.gate1 = take(2)                 # conv_s.1, conv_t.1
        s.tower1 = take(4)                # first tower level (dropout-free)
        s.res = take((0 if isinstance(m.dsgn.residual, nn.Identity) else 2) + (0 if isinstance(m.residual, nn.Identity) else 1))
        s.gate5 = take(2)                 # conv_s.5, conv_t.5
        s.tower4 = take(4)                # time_compress.4, joint_compress.4 of either Map2Adj
        s.gate_map = take(2)              # map_s.1, map_t.1
        s.expansor = take(2)
        s.tcn = take(2)
        s.tail = take(4)                  # prelu1.0, prelu2.0, compressor.1, the gated output (dropout-free)
        if self.drop_trace is not None:
            towers4 = [t[4] for d in doms for t in (d.map_to_adj.time_compress, d.map_to_adj.joint_compress)]
            for mods, ids in (((m.conv_s[1], m.conv_t[1]), s.gate1), ((m.conv_s[5], m.conv_t[5]), s.gate5), (towers4, s.tower4),
                              ((m.map_s[1], m.map_t[1]), s.gate_map), ([d.map_to_adj.expansor[1] for d in doms], s.expansor),
                              ([d.tcn[1] for d in doms], s.tcn)):
                self.drop_trace.update(zip(mods, ids))
        return s

    @staticmethod
    def _branches(m, p):
        """One record per branch of the block; each stage adds its result under the stage's name.
        gate[i] (space, time): rows -> act -> cols (-> hidden on the row-kernel chain); tower[k] (time, joint of dsgn, then of tsgn):
        map -> act (with `transform` when deferred) -> col -> norm -> out; res: maps -> dom[0..1], block."""
        gate = [SimpleNamespace(conv=c, lin=l) for c, l in ((m.conv_s, m.map_s), (m.conv_t, m.map_t))]
        pairs = [tuple(SimpleNamespace(net=t, rows=rows, transform=None) for t, rows in ((d.map_to_adj.time_compress, True), (d.map_to_adj.joint_compress, False)))
                 for d in (m.dsgn, m.tsgn)]
        tower = [tw for pair in pairs for tw in pair]
        for tw, ok in zip(tower, p.collapse):
            tw.collapse = ok
        return SimpleNamespace(gate=gate, tower=tower, pairs=pairs, res=SimpleNamespace())

    def _stage_input(self, m, p, s, x):
        """global_norm, the block statistics and one alias of the normalised input per consumer - the statistics, the first-level maps,
        both graph stages and the identity residuals -, so that backward sums their gradients in one launch (ops.fanout)"""
        n_alias = 4 + int(p.stacked) + int(p.rows_gate) + len(p.res_groups or ()) + (0 if p.has_res else 2) + (0 if p.has_bres else 1)
        if p.fused_in:
            # global_norm and the block statistics from one pass over the block input; in backward the gradients of all the consumers below,
            # the statistics' gradient and the BatchNorm backward are two streaming passes (csrc/block_input.hip)
            x_in, x_sums = x if isinstance(x, tuple) else (x, None)
            xa, gate_stats = ops.block_input(x_in, m.global_norm, p.tr, n_alias - 1, stats=x_sums if p.tr else None)
            xa = iter([None] + list(xa))
        else:
            xa = iter(ops.fanout(self._na(x, bn=m.global_norm, salt=s.global_norm), n_alias))
        xs = SimpleNamespace(stats=next(xa), norm=next(xa), dom=(next(xa), next(xa)))
        xs.maps = next(xa) if p.stacked else None
        xs.gates = next(xa) if p.rows_gate else None
        xs.resmaps = [next(xa) for _ in p.res_groups or ()]
        xs.res = None if p.has_res else (next(xa), next(xa))
        xs.bres = None if p.has_bres else next(xa)
        if not p.fused_in:
            gate_stats = ops.fanout(ops.dstd_stats(xs.stats), 2)      # one alias per gate path
        xs.gate_stats = tuple(gate_stats)
        return xs

    def _stage_maps(self, p, br, xs):
        """1. every first-level map of xn: contraction items in the order gates | towers | residual maps, less what a stacked kernel takes"""
        tr, xn = p.tr, xs.norm
        cs, ct = br.gate[0].conv[0], br.gate[1].conv[0]
        items, gate_rows = [], None
        if p.gates:
            O = cs.out_channels
            w2 = ops.cat_channels([cs.weight.view(1, O, -1), ct.weight.view(1, O, -1)]).view(2 * O, cs.in_channels, xn.shape[2])
            if p.rows_gate:
                gate_rows, br.gate_sums = ops.collapse_rows(xs.gates, w2, p.mid_g and tr)      # whole-sample kernel (csrc/collapse_rows.hip)
            else:
                items = [(("och,bchw->bow", w2, xn, None, None, None), None)]
        else:
            items = [_rows_item(xn, cs, tr), _rows_item(xn, ct, tr)]
        if not p.stacked:
            items += [_pw_item(xn, tw.net[0], tr) for tw in br.tower]
        if p.res_groups is None:
            items += [_pw_item(xn, c, tr) for c in p.res_convs]
        out = iter(_run_items(items) if items else [])
        if p.gates:
            yg = gate_rows if p.rows_gate else next(out)[0]
            for g, y in zip(br.gate, ops.split_channels(yg, (O, O))):
                g.rows = (y.unsqueeze(2), None)
        else:
            for g in br.gate:
                g.rows = next(out)
        bns, prelus = [tw.net[1] for tw in br.tower], [tw.net[2] for tw in br.tower]
        if p.defer:
            raw, transforms = ops.tower_maps(xs.maps, p.tower_w, bns, prelus, tr, defer=True)
            for tw, y, t in zip(br.tower, raw, transforms):
                tw.act, tw.transform = y, t              # the raw map: its collapsing kernel normalises and activates on load
                if self.act_trace is not None:           # branch records: the collapsing kernels write the activated maps out as well
                    t["want_tap"] = True
        elif p.tower_fused:
            for tw, h in zip(br.tower, ops.tower_maps(xs.maps, p.tower_w, bns, prelus, tr)):
                tw.act = h
                if self.act_trace is not None:
                    self.act_trace[tw.net[2]] = (h.detach(), None)
        else:
            ys = ops.pointwise_maps(xs.maps, p.tower_w, tr) if p.stacked else [next(out) for _ in br.tower]
            for tw, y in zip(br.tower, ys):
                tw.map = y
        res_biases = [c.bias for c in p.res_convs]
        if p.res_groups is None:
            br.res.maps = list(out)
        else:
            # per group; `maps` holds the finished residuals when the group operator applies the BatchNorm too (p.res_fused)
            br.res.maps = [None] * len(p.res_convs)
            for xg, grp in zip(xs.resmaps, p.res_groups):
                ws, bs = [p.res_w[i] for i in grp], [res_biases[i] for i in grp]
                ys = (ops.tower_maps(xg, ws, [p.res_bns[i] for i in grp], [None] * len(grp), tr, biases=bs) if p.res_fused
                      else ops.pointwise_maps(xg, ws, tr, biases=bs))
                for i, y in zip(grp, ys):
                    br.res.maps[i] = y

    def _stage_map_tails(self, p, s, br, xs):
        """2. BatchNorm / PReLU tails of the first-level maps, for the branches whose kernel has not applied them already.  (The gates'
        conv_s.1 / conv_t.1 with their Dropout and PReLU run inside ops.block_mid when `p.mid_g`.)"""
        gates = [] if p.mid_g else [dict(x=g.rows, bn=g.conv[1], drop=True, prelu=g.conv[3], salt=sid) for g, sid in zip(br.gate, s.gate1)]
        towers = [] if p.tower_fused else [dict(x=tw.map, bn=tw.net[1], prelu=tw.net[2], salt=sid) for tw, sid in zip(br.tower, s.tower1)]
        res = [] if p.res_fused else [dict(x=y, bn=bn, salt=sid) for y, bn, sid in zip(br.res.maps, p.res_bns, s.res)]
        if p.tower_fused:                # the towers' operator ran between the gates' maps and the residual ones: a launch on either side
            out = iter((self._na_many(gates) if gates else []) + (self._na_many(res) if res else []))
        else:
            out = iter(self._na_many(gates + towers + res))
        if gates:
            for g in br.gate:
                g.act = next(out)
        if towers:
            for tw in br.tower:
                tw.act = next(out)
        done = iter(br.res.maps if p.res_fused else out)
        br.res.dom = (next(done), next(done)) if p.has_res else xs.res
        br.res.block = next(done) if p.has_bres else xs.bres

    def _stage_collapse(self, p, br):
        """3. collapsing convolutions: the gates' (1,V) ones and the towers' (T,1) / (1,V) ones; a tower inside the limits of the
        whole-sample kernels takes its own launch, the rest share one contraction launch (order gates | towers)"""
        tr = p.tr
        items = [] if p.mid_g else [_cols_item(g.act, g.conv[4], tr) for g in br.gate]
        for tw in br.tower:
            c = tw.net[3]
            if tw.collapse:
                x3 = tw.act[0] if isinstance(tw.act, tuple) else tw.act
                w3 = c.weight.view(c.out_channels, c.in_channels, -1)
                if tw.rows:
                    y, st = ops.collapse_rows(x3, w3, tr, transform=tw.transform)      # whole-sample kernel (csrc/collapse_rows.hip)
                else:
                    y, st = ops.collapse_cols(x3, w3, tr, transform=tw.transform)      # whole-sample kernel for the joint axis
                tw.col = (y.unsqueeze(2 if tw.rows else 3), st)
            else:
                items.append((_rows_item if tw.rows else _cols_item)(tw.act, c, tr))
        if p.defer and self.act_trace is not None:
            for tw in br.tower:
                self.act_trace[tw.net[2]] = (tw.transform["tap"].detach(), None)
        out = iter(_run_items(items) if items else [])
        for g in [] if p.mid_g else br.gate:
            g.cols = next(out)
        for tw in br.tower:
            if not tw.collapse:
                tw.col = next(out)

    def _stage_mid_chain(self, p, s, br, xs):
        """4. / 5. on the row-kernel chain (a gate path outside ops.gate_head_ok): BatchNorm tails of gates and towers in one launch, the
        gates' first Linear and the last tower maps in one contraction launch, then map_s.1 / map_t.1; `hidden` waits for its last Linear"""
        tr = p.tr
        calls = [dict(x=g.cols, bn=g.conv[5], drop=True, prelu=g.conv[7], salt=sid) for g, sid in zip(br.gate, s.gate5)]
        calls += [dict(x=tw.col, bn=tw.net[4], drop=True, salt=sid) for tw, sid in zip(br.tower, s.tower4)]
        r = iter(self._na_many(calls))
        items = [_lin_item(ops.cat_channels([next(r).view(p.B, -1), st]), g.lin[0], tr) for g, st in zip(br.gate, xs.gate_stats)]
        for tw in br.tower:
            tw.norm = next(r)
        items += [_pw_item(tw.norm, tw.net[6], False) for tw in br.tower]
        out = iter(_run_items(items))
        lin = [next(out) for _ in br.gate]
        for tw in br.tower:
            tw.out = next(out)
        hidden = self._na_many([dict(x=y, bn=g.lin[1], drop=True, prelu=g.lin[3], salt=sid) for y, g, sid in zip(lin, br.gate, s.gate_map)])
        for g, h in zip(br.gate, hidden):
            g.hidden = h

    def _stage_mid(self, m, p, s, br, xs):
        """4. / 5. with the gate head: the towers' BatchNorm tails, then everything of the two gate paths behind their (1,V) convolutions
        in one launch (csrc/gate_head.hip), then the last tower maps.  ops.block_mid (csrc/block_mid.hip) takes the gates' mid-section
        (`p.mid_g`) and the towers' tails with their last maps (`p.mid_t`) into one launch in front of the gate head."""
        tr, B, V = p.tr, p.B, p.V
        Cg = m.conv_s[4].out_channels
        if not p.mid_t:
            norms = self._na_many([dict(x=tw.col, bn=tw.net[4], drop=True, salt=sid) for tw, sid in zip(br.tower, s.tower4)])
            for tw, h in zip(br.tower, norms):
                tw.norm = h
        if p.mid_g or p.mid_t:
            # gates: BatchNorm -> Dropout -> PReLU -> (1,V) convolution; towers: BatchNorm -> Dropout -> last 1x1 map: one launch, two backward
            items = []
            if p.mid_g:
                for i, (g, sid) in enumerate(zip(br.gate, s.gate1)):
                    x1 = g.rows[0].squeeze(2)
                    items.append(dict(kind=0, x=x1, bn=g.conv[1], prelu=g.conv[3], weight=g.conv[4].weight.view(Cg, -1, V), salt=sid,
                                      stats=(br.gate_sums, i * x1.shape[1], 2 * x1.shape[1]) if tr else None))
            if p.mid_t:
                for tw, sid in zip(br.tower, s.tower4):
                    (y, st), c = tw.col, tw.net[6]
                    items.append(dict(kind=1, x=y.view(B, y.shape[1], -1), bn=tw.net[4], prelu=None, weight=c.weight.view(c.out_channels, y.shape[1]),
                                      salt=sid, stats=(st, 0, y.shape[1]) if tr else None))
            taps = [] if self.act_trace is not None else None
            out = iter(ops.block_mid(items, tr, drop_p=self.dropout, taps=taps))
            if p.mid_g:
                for g in br.gate:
                    g.cols = (next(out), None)
                if taps is not None:
                    self.act_trace[m.conv_s[3]], self.act_trace[m.conv_t[3]] = (taps[0].unsqueeze(2), None), (taps[1].unsqueeze(2), None)
            if p.mid_t:
                for tw in br.tower:
                    tw.out = (next(out), None)
        # the site ids are the ones the row-kernel chain numbers: conv_s.5 / conv_t.5 in front of the four tower sites, map_s.1 / map_t.1 behind them
        taps = [] if self.act_trace is not None else None
        m.w1, m.w2 = ops.gate_head([g.cols[0].view(B, Cg) for g in br.gate], list(xs.gate_stats), [m.conv_s, m.conv_t], [m.map_s, m.map_t], tr,
                                   drop_p=self.dropout, salts=tuple(zip(s.gate5, s.gate_map)), taps=taps)
        if taps is not None:
            self.act_trace[m.conv_s[7]], self.act_trace[m.map_s[3]] = (taps[0], None), (taps[1], None)
            self.act_trace[m.conv_t[7]], self.act_trace[m.map_t[3]] = (taps[2], None), (taps[3], None)
        if not p.mid_t:
            for tw, y in zip(br.tower, _run_items([_pw_item(tw.norm, tw.net[6], False) for tw in br.tower])):
                tw.out = y

    def _stage_adjacency(self, m, p, s, br):
        """6. / 7. the Map2Adj seeds  o[b,v,t,tau] = s[b,v,t] q[b,tau,v]  |  o[b,t,v,w] = s[b,v,t] q[b,t,w]  of the tower pairs and
        their expansors -> [Adj of dsgn, Adj of tsgn]; a gate path on the row-kernel chain gets its output Linear here (m.w1, m.w2)"""
        tr, B, T, V = p.tr, p.B, p.T, p.V
        doms = (m.dsgn, m.tsgn)
        expansors = [d.map_to_adj.expansor for d in doms]
        seeds = [(0 if d.domain == "space" else 1, joint.out[0].view(B, V, T), time.out[0].view(B, T, V)) for d, (time, joint) in zip(doms, br.pairs)]
        last = [] if p.gate_fused else [_lin_item(g.hidden, g.lin[4], False) for g in br.gate]
        if p.adj_fused:
            # seed, expansor and adjacency of both towers in two phase launches (csrc/map2adj_tail.hip); the seed is never stored
            if last:
                (m.w1, _), (m.w2, _) = _run_items(last)
            taps = [] if self.act_trace is not None else None
            adj = ops.map2adj_tail(seeds, expansors, tr, drop_p=self.dropout, salts=s.expansor, taps=taps)
            if taps is not None:
                for e, tap in zip(expansors, taps):
                    self.act_trace[e[3]] = (tap, None)
            return list(adj)
        if T <= 64 and V <= 64:
            oo = ops.rank1_adj(seeds)                        # both towers in one launch; backward reads each d o once
        else:
            oo = [y for y, _ in ops.contract_many([("bvt,bxv->bvtx" if dom == 0 else "bvt,btw->btvw", sv, q, None, None, None) for dom, sv, q in seeds])]
        # 7. gate output Linear + expansor first map
        out = iter(_run_items(last + [_pw_item(o, e[0], tr) for o, e in zip(oo, expansors)]))
        if last:
            m.w1, m.w2 = next(out)[0], next(out)[0]
        h = self._na_many([dict(x=next(out), bn=e[1], drop=True, prelu=e[3], salt=sid) for e, sid in zip(expansors, s.expansor)])
        return [y for y, _ in _run_items([_pw_item(hi, e[4], False) for hi, e in zip(h, expansors)])]

    def _stage_graph_tail(self, m, p, s, br, xs, adj):
        """8. graph product + channel mix of both domain layers, then everything behind them: BatchNorm + residual + PReLU, gates,
        compressor, squeeze-excite, block residual.  Returns the block output, in train mode with its f64 channel sums."""
        tr = p.tr
        doms = (m.dsgn, m.tsgn)
        res, bres = br.res.dom, br.res.block
        ys = []
        for d, x_dom, a, fused in zip(doms, xs.dom, adj, p.stage_fused):
            d.Adj = a
            conv = d.tcn[0]
            if fused:
                wmat = conv.weight.view(conv.out_channels, conv.in_channels)
                ys.append(ops.stgcn_domain(x_dom, d.Adj, wmat, conv.bias, 0 if d.domain == "space" else 1, tr))
            else:
                spec = "bctv,bvtq->bcqv" if d.domain == "space" else "bctv,btvw->bctw"
                ys.append(self._lin(_pointwise, ops.contract(spec, x_dom, d.Adj), conv))
        c = m.compressor
        # (a generic contraction that had to split K comes without channel sums: only the call itself tells)
        if p.tail_fused and all(st is not None or not tr for _, st in ys):
            # everything behind the two tcn convolutions in five phase launches (csrc/dstd_tail.hip); the four (dropout-free) sites of
            # the row-kernel chain below stay unused
            taps = [] if self.act_trace is not None else None
            rs_shared = not p.has_res and res[0].data_ptr() == res[1].data_ptr()      # identity residuals: one summed gradient
            alphas = (doms[0].prelu, doms[1].prelu, m.prelu1[1], m.prelu2[1], c[2])
            out, ost = ops.dstd_tail([y for y, _ in ys], [st for _, st in ys], res, (m.w1, m.w2),
                                     (doms[0].tcn[1], doms[1].tcn[1], m.prelu1[0], m.prelu2[0], c[1]), alphas, c[0].weight, c[3], bres, tr,
                                     drop_p=self.dropout, salts=s.tcn, emit_stats=tr, taps=taps, rs_shared=rs_shared)
            if taps is not None:
                for mod, tap in zip(alphas, taps):
                    self.act_trace[mod] = (tap, None)
            return (out, ost) if tr else out
        s_prelu1, s_prelu2, s_compressor, s_out = s.tail
        x12 = self._na_many([dict(x=y, bn=d.tcn[1], drop=True, add=r, prelu=d.prelu, salt=sid) for y, d, r, sid in zip(ys, doms, res, s.tcn)])
        ab = self._na_many([dict(x=x12[0], pre=m.w1, bn=m.prelu1[0], prelu=m.prelu1[1], salt=s_prelu1),
                            dict(x=x12[1], pre=m.w2, bn=m.prelu2[0], prelu=m.prelu2[1], salt=s_prelu2)])
        h = self._na(self._lin(_pointwise, ops.cat_channels(ab), c[0]), bn=c[1], prelu=c[2], salt=s_compressor)
        h_pool, h = ops.fanout(h, 2)                                     # squeeze | excite
        gate = ops.se_gate(ops.mean_bc(h_pool), c[3].w1, c[3].w2)
        # the next block starts with a BatchNorm of this output: let the kernel emit its channel sums (train mode)
        return self._na(h, pre=gate, add=bres, add_post=True, emit_stats=tr, salt=s_out)

    # ---- FPN.forward, CISTGCN.py:74-79 -------------------------------------------------------------
    def _fpn(self, m, x, x_pool=None):
        blocks = (m.block1, m.block2, m.block3)
        ys = ops.dilated_convs(x, [b[0] for b in blocks])
        outs = self._na_many([dict(x=y, bn=b[1], prelu=b[3]) for y, b in zip(ys, blocks)])   # FPN dropout p = 0 (:533)
        outs.append(ops.mean_bc(x if x_pool is None else x_pool))                  # action context, broadcast below
        return _pointwise(ops.cat_channels(outs, bcast=(False, False, False, True)), m.compress)[0]

    # ---- ContextLayer.forward, CISTGCN.py:463-475 --------------------------------------------------
    def _context(self, m, x7):
        B, To, V, _ = x7.shape
        x = x7.view(B, 1, To, V * 3)
        c1, c2, c3 = m.context_conv1, m.context_conv2, m.context_conv3
        tr = self.training
        w13 = [c[0].weight.view(c[0].out_channels, c[0].in_channels) for c in (c1, c3)]
        if c1[0].bias is None and c3[0].bias is None and ops.context_heads_ok(x, c1[0].out_channels):
            # heads 1 and 3 (max / mean over the positions of a 1 -> hidden_dim map, BatchNorm, PReLU) from the one-channel sequence
            # itself: their (B, hidden_dim, To, 3V) activations are never stored (csrc/context_heads.hip)
            xa, xb = ops.fanout(x, 2)
            taps = [] if self.act_trace is not None else None
            y1, ym = ops.context_heads(xa, c1, c3, tr, taps=taps)
            if taps is not None:
                self.act_trace[c1[2]], self.act_trace[c3[2]] = (taps[0], None), (taps[1], None)
            y2 = ops.max_bc(self._na(_run_items([_rows_item(xb, c2[0], tr)])[0], bn=c2[1], prelu=c2[2]))
            self._site += 2          # the composite path numbers two more (dropout-free) sites: later layers draw the same masks on either path
            return self._context_tail(m, x7, y1, y2, ym)
        if self.fused_maps and B * To * V * 3 * sum(w.shape[0] for w in w13) >= self.stack_min_elements and ops.pointwise_maps_ok(x, w13):
            # the two 1 -> hidden_dim maps read the sequence once and write their (B, hidden_dim, To, 3V) results from one kernel
            xa, xb = ops.fanout(x, 2)
            y13 = ops.pointwise_maps(xa, w13, tr, biases=[c1[0].bias, c3[0].bias])
            o = [y13[0], _run_items([_rows_item(xb, c2[0], tr)])[0], y13[1]]
        else:
            o = _run_items([_pw_item(x, c1[0], tr), _rows_item(x, c2[0], tr), _pw_item(x, c3[0], tr)])
        r = self._na_many([dict(x=o[i], bn=c[1], prelu=c[2]) for i, c in enumerate((c1, c2, c3))])
        return self._context_tail(m, x7, ops.max_bc(r[0]), ops.max_bc(r[1]), ops.mean_bc(r[2]))

    def _context_tail(self, m, x7, y1, y2, ym):
        """ContextLayer.forward behind the three pooled heads, CISTGCN.py:468-475"""
        B, To, V, _ = x7.shape
        tr = self.training
        o = _run_items([_lin_item(y, h[0], False) for y, h in ((y1, m.map1), (y2, m.map2), (ym, m.map3))])
        heads = self._na_many([dict(x=o[i][0], drop=True, prelu=h[2]) for i, h in enumerate((m.map1, m.map2, m.map3))])
        y = ops.cat_channels(heads)
        o = _run_items([_lin_item(y, m.fmap_s[0], tr), _lin_item(y, m.fmap_t[0], tr)])
        m.joints, m.displacements = self._na_many([dict(x=o[0], bn=m.fmap_s[1], drop=True), dict(x=o[1], bn=m.fmap_t[1], drop=True)])
        m.seq_joints = ops.contract("bt,bv->btv", m.displacements, m.joints)
        n = m.norm_map
        h = self._na(self._lin(_pointwise, m.seq_joints, n[0]), bn=n[1], drop=True, prelu=n[3])
        h_pool, h = ops.fanout(h, 2)
        h = self._na(h, pre=ops.se_gate(ops.mean_bc(h_pool), n[4].w1, n[4].w2))
        h = self._na(self._lin(_pointwise, h, n[5]), bn=n[6], drop=True, prelu=n[8])
        m.seq_joints_n = h
        f = m.fconv
        h = self._na(self._lin(_pointwise, h.view(B, 1, To, V), f[0]), bn=f[1], prelu=f[2])
        h = self._na(self._lin(_pointwise, h, f[3]), bn=f[4], prelu=f[5])
        m.seq_joints_dims = h
        hp_pool, hp = ops.fanout(h.permute(0, 2, 3, 1), 2)
        return self._na(hp, pre=ops.se_gate(ops.mean_bc(hp_pool), m.SE.w1, m.SE.w2))

    # ---- CISTGCN.forward, CISTGCN.py:567-597 -------------------------------------------------------
    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != self.n_input or x.shape[2] != self.n_joints or x.shape[3] != 3:
            raise ValueError("expected input of shape (B, %d, %d, 3), got %s" % (self.n_input, self.n_joints, tuple(x.shape)))
        if torch.jit.is_tracing():
            # `SummaryWriter.add_graph(model, batch)` (train.py:137) traces the model.  The kernels are reached through ctypes and
            # exchange statistics buffers the tracer cannot follow, so the hot path is shown to it as ONE opaque node.
            net = self

            class HotPath(torch.autograd.Function):
                @staticmethod
                def forward(ctx, inp):
                    state = torch._C._get_tracing_state()
                    torch._C._set_tracing_state(None)          # nothing inside is recorded
                    try:
                        with torch.no_grad():
                            return net._forward(inp.detach(), bump_seed=False)[0]
                    finally:
                        torch._C._set_tracing_state(state)

                @staticmethod
                def backward(ctx, g):
                    raise RuntimeError("the traced CISTGCN graph is for display only")

            return HotPath.apply(x),
        return self._forward(x, bump_seed=self.training and self.dropout > 0.0)

    def _forward(self, x, bump_seed):
        ops.begin_step(x.device, bump_seed=bump_seed)
        self._site, self._next_stream = 0, 0
        h = ops.feature_lift(x)                                         # (B,10,T,V)
        block = self._block_staged if self.staged else self._block
        for i, blk in enumerate(self.st_gcnns):
            h = block(blk, h)
            if self.backward_cut is not None and self.backward_cut[0] == i:
                h = self.backward_cut[1](h)                               # runtime.DataParallelStep: two-phase backward
        h = h[0] if isinstance(h, tuple) else h                          # (tensor, channel sums) from a staged block
        h = h.permute(0, 2, 1, 3)                                       # NCTV -> NTCV (view)
        ha = ops.fanout(h, 2)                                           # dilated convolutions | pooled context
        z = self._na(self._fpn(self.txcnns[0], ha[0], ha[1]), prelu=self.prelus[0])
        for i in range(1, self.n_txcnn_layers):
            za = ops.fanout(z, 3)                                       # ... | skip connection
            z = self._na(self._fpn(self.txcnns[i], za[0], za[1]), prelu=self.prelus[i], add=za[2], add_post=True)
        d = self.dim_conversor
        z = self._na(self._lin(_pointwise, z.permute(0, 2, 1, 3), d[0]), bn=d[1], prelu=d[2])
        z = self._na(_pointwise(z, d[3])[0], prelu=d[4])                # PReLU(3): per-channel slopes (:545)
        x7, x7o = ops.fanout(ops.cumsum_time(z.permute(0, 2, 3, 1)), 2)   # (B,T_out,V,3): context branch | output block
        def output_blocks():
            x8 = x7o.permute(0, 3, 2, 1)                                # (B,3,V,T_out) view
            for blk in self.st_gcnns_o:
                x8 = block(blk, x8)
            return x8[0] if isinstance(x8, tuple) else x8
        act, x8 = self._parallel([lambda: self._context(self.context_layer, x7), output_blocks], [x7])
        return ops.add3(x[:, -1:], x8.permute(0, 3, 2, 1), act),
